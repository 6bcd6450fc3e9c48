"""Why the GPU tests of the long single-token attention forms can be trusted (no GPU): the plan of the split-KV flash form leaves whole splits without a live
position at every shape, the emulation of the right algorithm under that plan is inside fattn_model's bound at every element of every case, a kernel that
ignores the device-side position count or merges an empty partial with weight 1 is outside it at every row it touches (and so are the maskless mutants of
test_fattn_model.py); the soft-max boundary rows meet their condition and the numpy restatement behind them has the oracle's words; and the random rows of the
old soft-max test never took the branch."""
import numpy as np
import pytest

import attn_long_model as AL
import fattn_model as FM
import oracle as O
from test_fattn_model import ratio_of, rows_outside


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_long_flash_plan_follows_the_launcher():
    assert AL.long_flash_plan(8, 128, 1024) == (True, 128, 8)                  # room for 10 partials per head: 16 tiles go two to a split
    assert AL.long_flash_plan(8, 128, 2112) == (True, 128, 17)                 # 33 tiles: the last split is one tile
    assert AL.long_flash_plan(8, 64, 1024) == (True, 64, 16) and AL.long_flash_plan(4, 64, 2112) == (True, 64, 33)
    assert AL.long_flash_plan(32, 128, 16384) == (True, 512, 32)               # per = tiles / 32
    assert AL.long_flash_plan(8, 128, 1024, s_bytes=4096) is None              # no room beside the rotated query
    assert AL.long_flash_plan(8, 128, 1024, s_bytes=4096 + 3 * 8 * 132 * 4) is None and AL.long_flash_plan(8, 128, 1024, s_bytes=4096 + 4 * 8 * 132 * 4) == (True, 256, 4)
    assert AL.long_flash_plan(64, 64, 1024, nkv=1) is None                     # r2 > 32
    assert AL.long_flash_plan(8, 96, 1024) is None and AL.long_flash_plan(8, 128, 1028) is None
    assert AL.decode_wsize(32, 2048) == 32 * 2048 * 6                          # test_rope_kv_attn_decode_rejects_what_it_cannot_do pins the library's to the same


@pytest.mark.parametrize("shape", AL.FLASH_SHAPES, ids=str)
@pytest.mark.parametrize("ML", AL.FLASH_ML)
def test_every_flash_shape_has_a_split_with_no_live_position(shape, ML):
    hd, nh, nkv, mode = shape
    decode, chunk, splits = AL.long_flash_plan(nh, hd, ML, AL.decode_wsize(nh, ML), nkv)
    assert decode and 4 <= splits <= 256 and splits * chunk >= ML and chunk % 64 == 0
    for n_kv in AL.flash_n_kv(ML):
        live = (n_kv + chunk - 1) // chunk
        if n_kv in (513, 576, 577):
            assert live < splits                                                # (n_kv = ML - 1 and ML fill every split: the ragged last one)


# ---- the right algorithm passes, the wrong ones do not ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AL.FLASH_CASES, ids=AL.flash_id)
def test_flash_emulation_is_inside_the_bound_and_the_long_mutants_are_not(case):
    hd, nh, nkv, mode, ML, n_kv, prof = case
    d = AL.flash_case_data(case)
    ref, (_, chunk, splits) = d["ref"], d["plan"]
    out, info = AL.emulate_flash_case(case)
    ratio = ratio_of(out, ref)
    print(f"emulation |got - R| / bound: {ratio.max():.3f} {AL.flash_id(case)}")
    assert np.all(np.isfinite(out)) and np.all(ratio <= 1.0), float(ratio.max())
    live = ref["A"] > 0
    assert np.all(ref["n_vis"] == n_kv) and np.all(live)
    # the operands the kernel gets past n_kv are the poison: V NaN, K of exponent 2^14
    if n_kv < ML:
        assert np.all(np.isnan(d["Vop"][0, :, n_kv:])) and np.all((np.abs(d["Kop"][0, :, n_kv:]) >= 2.0 ** 14) & (np.abs(d["Kop"][0, :, n_kv:]) < 2.0 ** 15))
        mut, _ = AL.emulate_flash_case(case, ["ignore_n_kv_dev"])
        assert np.all(rows_outside(mut, ref))
    empty = splits - (n_kv + chunk - 1) // chunk
    if empty:
        mut, _ = AL.emulate_flash_case(case, ["empty_split_weight_1"])
        assert np.all(rows_outside(mut, ref)), int(empty)
    # the profile keeps its promise under the long plan: merge weights far from 1
    if prof == "split_maxima":
        assert np.all(info["wmin"] < -40)
    if prof == "ascending":
        assert np.all(info["wmin"] < -2 * FM.FA_TAU)


def _group_edge_heads(case, info, ref):
    H, r = case[1], case[1] // case[2]
    t = np.zeros(ref["n_vis"].shape, bool)
    t[:, :, [h for h in range(H) if ((h + 1) % H) // r != h // r]] = True
    return t


_resc = lambda case, info, ref: info["rescales"] >= 1
_all = lambda case, info, ref: ref["n_vis"] > 0
# the mutants of fattn_model.MUTATIONS that apply without a mask, on cases of the long plan (profile named in the case)
LONG_MUTANTS = [
    ("no_l_rescale", [(128, 8, 2, 0, 1024, 577, "ascending"), (128, 16, 2, 2, 2112, 577, "ascending")], _resc),       # (the last live split holds two tiles: its rescale decides the result)
    ("no_o_rescale", [(128, 8, 2, 0, 1024, 577, "ascending"), (128, 16, 2, 2, 2112, 577, "ascending")], _resc),
    ("drop_last_ragged", [(128, 8, 2, 0, 1024, 577, "ascending"), (128, 16, 2, 2, 2112, 513, "ascending")], _all),
    ("merge_w1", [(128, 8, 2, 0, 1024, 577, "split_maxima"), (128, 8, 8, 2, 2112, 2112, "ascending")], _all),
    ("merge_l_unweighted", [(128, 8, 2, 0, 1024, 577, "split_maxima"), (64, 4, 1, 2, 2112, 2111, "ascending")], _all),
    ("kv_head_next", [(128, 8, 2, 0, 1024, 577, "gaussian"), (128, 16, 2, 2, 2112, 2112, "gaussian")], _group_edge_heads),
]


@pytest.mark.parametrize("mutation,cases,touched", LONG_MUTANTS, ids=[m[0] for m in LONG_MUTANTS])
def test_maskless_mutants_stay_outside_the_bound_under_the_long_plan(mutation, cases, touched):
    for case in cases:
        assert case in AL.FLASH_CASES
        ref = AL.flash_case_data(case)["ref"]
        _, info = AL.emulate_flash_case(case)
        out, _ = AL.emulate_flash_case(case, [mutation])
        t = touched(case, info, ref)
        assert t.sum() >= 1, case
        bad = rows_outside(out, ref)
        assert np.all(bad[t]), (case, int(t.sum()), int((t & ~bad).sum()))


# ---- the soft-max boundary rows ------------------------------------------------------------------------------------------------------------
def test_the_restated_expf_is_the_oracle_s():
    r = np.random.default_rng(5)
    x = np.concatenate([r.uniform(-104.0, 90.0, 20000), r.uniform(-20.0, 0.0, 40000), -np.exp(r.uniform(-20.0, 3.0, 20000)), [0.0, -0.0, -87.0, -88.5, -126.5, 88.0]]).astype(np.float32)
    L = O.lib()
    want = np.array([L.orc_expf_avx2(float(v)) for v in x], np.float32)
    assert np.array_equal(AL.v_expf(x).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", [64, 513, 1000, 1024, 4097])
def test_boundary_rows_meet_the_condition_and_the_restatement_has_the_oracle_s_words(n):
    rows = 3
    x, deciding = AL.boundary_rows(n, rows, 0)
    want = np.zeros((rows, n), np.float32)
    O.soft_max(O.tensor(np.array(x), O.F32, [n, rows]), None, O.tensor(want, O.F32, [n, rows]))
    for i in range(rows):
        e = AL.soft_max_terms(x[i])
        assert AL.boundary_distance(AL.serial_total(e))[0] <= AL.half_window(n)
        assert np.array_equal(AL.soft_max_restated(x[i]).view(np.uint32), want[i].view(np.uint32))
        # a tree total stays inside the kernels' whole window (m + 24): they all take the fallback
        assert AL.boundary_distance(AL.pairwise_total(e))[0] <= (n >> 3) + 24
    print(f"n = {n}: {int(deciding.sum())} of {rows} rows are order-deciding")


def test_random_soft_max_rows_are_never_on_a_boundary():
    """rows of the distribution test_gpu_ops.test_soft_max draws from (3 N(0, 1); not its very draws: that test shares a generator with the tests before it): none
    in the window -- the expected number is ~1e-5 -- so rows like these do not take the branch"""
    rng = np.random.default_rng(11)
    hit = 0
    for n0 in (8, 33, 1024, 4097):
        x = (rng.standard_normal((2, 3, n0)) * 3).astype(np.float32).reshape(-1, n0)
        hit += sum(AL.boundary_distance(AL.pairwise_total(AL.soft_max_terms(r)))[0] <= (n0 >> 3) + 24 for r in x)
    assert hit == 0


@pytest.mark.parametrize("shape", AL.BOUNDARY_ATTN, ids=str)
def test_attn_boundary_case_has_a_hit_head(shape):
    hd, nh, nkv, ML, n_past, mode = shape
    d = AL.boundary_attn_case(shape)
    assert len(d["hits"]) >= 1 and d["j"] < n_past
    for h in d["hits"]:
        e = AL.soft_max_terms(d["oracle"]["scores"][h])
        assert AL.boundary_distance(AL.serial_total(e))[0] <= AL.half_window(n_past + 1)
        assert np.array_equal(AL.soft_max_restated(d["oracle"]["scores"][h]).view(np.uint32), d["oracle"]["p"][h].view(np.uint32))
    row = d["kc0"][d["j"]].reshape(nkv, hd).astype(np.float32)
    assert sum(int(np.count_nonzero(g) == 2) for g in row) == 1                  # one kv head's row: two non-zero entries
    print(f"{shape}: heads {d['hits']} on a boundary")
