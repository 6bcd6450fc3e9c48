"""Why the bounds of tests/fattn_model.py can be trusted (no GPU): the operand mirror is pinned to the oracle, the float64 reference agrees with the oracle's
flash attention, the step-by-step emulation of the right algorithm is inside the bound at every element of every case the GPU tests run, the score profiles
drive the paths they claim to (the lazy rescale, p > 1, merge weights far from 1), every mutant is outside the bound at every row it touches, and the max-norm
check the bound replaces lets a mutant through."""
import numpy as np
import pytest

import oracle as O
import fattn_model as FM

FA_ORACLE, FA_EXACT = 2e-2, 2e-3             # tests/test_gpu_fattn.py
CASE = {FM.case_id(c): c for c in FM.CASES}


def ratio_of(out, ref):
    """|out - R| / bound per element; a bound of 0 (a row with nothing visible) admits exact zeros only"""
    err = np.abs(out.astype(np.float64) - ref["R"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ref["bound"] > 0, err / ref["bound"], np.where(err == 0, 0.0, np.inf))


def rows_outside(out, ref):
    """[B, N, H]: the row has an element that is NOT inside the bound (NaN counts as outside)"""
    return np.any(~(np.abs(out.astype(np.float64) - ref["R"]) <= ref["bound"]), axis=-1)


def visible_tiles(case):
    """[B, N, H, splits]: the number of 64-position tiles of each split in which the row sees a key"""
    d = FM.case_data(case)
    _, chunk, splits = d["plan"]
    vis = np.isfinite(d["ref"]["x2"])
    B, H, N, n_kv = vis.shape
    pad = np.zeros((B, H, N, splits * chunk), bool)
    pad[..., :n_kv] = vis
    return pad.reshape(B, H, N, splits, chunk // 64, 64).any(-1).sum(-1).transpose(0, 2, 1, 3)


# ---- the operands and the reference are the oracle's ---------------------------------------------------------------------------
def test_type_codes_and_launch_plan():
    assert (FM.F16, FM.Q8_0) == (O.F16, O.Q8_0)
    assert FM.launch_plan(1, 8, 2, 64) == (True, 64, 1) and FM.launch_plan(1, 8, 2, 65) == (True, 64, 2) and FM.launch_plan(1, 8, 2, 300) == (True, 64, 5)
    assert FM.launch_plan(1, 4, 4, 8128) == (True, 64, 127)                       # the most splits the default CLLM_FA_DIV gives: 128 tiles go two to a split
    assert FM.launch_plan(1, 4, 4, 8192) == (True, 128, 64)
    assert FM.launch_plan(8, 8, 2, 78)[0] and not FM.launch_plan(11, 6, 2, 81)[0]   # N r = 32 | 33
    assert FM.launch_plan(1, 8, 2, 300, scratch=False) == (True, 320, 1)


@pytest.mark.parametrize("D", [64, 128])
def test_operand_mirror_equals_the_oracle_then_one_fp16_rounding(D):
    """Q8_0: q_operand == fp16(dequantize(quantize_row_q8_0(q))), kv_operand == fp16(dequantize(blocks)), word for word, on Gaussian rows, steered rows, rows
    with a zero block and a huge one; the module's own quantizer (which builds the Q8_0 caches of the profiles) writes the oracle's bytes"""
    r = np.random.default_rng(D)
    x = (r.standard_normal((40, D)) * 1.5).astype(np.float32)
    x[1, :32] = 0.0
    x[2] *= 300.0
    x[3] *= 1e-6
    x[4:12] = FM.profile("ascending", D, 2, 4, 2, 191, 61, FM.Q8_0, 0, "causal")[0].reshape(-1, D)
    h16 = lambda a: a.astype(np.float16).astype(np.float64)
    assert np.array_equal(FM.q_operand(FM.F16, x), h16(x))
    got = FM.q_operand(FM.Q8_0, x)
    blocks = FM.q8_0_quantize(x)
    for i, row in enumerate(x):
        ob = O.quantize_q8_0(row)
        assert np.array_equal(blocks[i], ob), i
        want = h16(O.dequantize(O.Q8_0, ob, D))
        assert np.array_equal(got[i], want), i
        assert np.array_equal(FM.kv_operand(FM.Q8_0, ob), want), i
    from synth_helpers import rand_blocks
    rb = rand_blocks(O.Q8_0, 16, D, r)
    assert np.array_equal(FM.kv_operand(FM.Q8_0, rb), np.stack([h16(O.dequantize(O.Q8_0, b, D)) for b in rb]))
    k16 = r.standard_normal((3, D)).astype(np.float16)
    assert np.array_equal(FM.kv_operand(FM.F16, k16), k16.astype(np.float64))


@pytest.mark.parametrize("cid", ["fa-1-128-130-4-2-191-61-stairs7-bias-0", "fa-8-128-1-8-2-300-299-sink_mixed-causal-0"])
def test_reference_agrees_with_the_oracle(cid):
    """the oracle (the reference's one_chunk order, fp16 V accumulator for an F16 cache) against R, relative to max |out| as tests/test_gpu_fattn.py does"""
    api, kv_t, D, N, H, Hkv, n_kv, n_past, profs, mm, ML = case = CASE[cid]
    d = FM.case_data(case)
    out = np.zeros((N, H, D), np.float32)
    rb = O.row_size(kv_t, D)
    e = 2 if kv_t == O.F16 else 34
    kv = lambda a: O.tensor(np.ascontiguousarray(a[0]), kv_t, [D, n_kv, Hkv], nb=[e, rb, rb * n_kv, rb * n_kv * Hkv])
    O.flash_attn_ext(O.tensor(np.ascontiguousarray(d["q"][0]), O.F32, [D, N, H]), kv(d["k"]), kv(d["v"]),
                     O.tensor(np.ascontiguousarray(d["mask"]), O.F16, [n_kv, N]), O.tensor(out, O.F32, [D, H, N]), float(d["scale"]))
    R = d["ref"]["R"][0]
    assert np.max(np.abs(out - R)) / np.max(np.abs(R)) < FA_ORACLE
    if mm == "bias":
        assert np.all(R[N // 2] == 0.0) and np.all(out[N // 2] == 0.0)


# ---- the right algorithm passes, and the profiles do what they promise ---------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASE))
def test_emulation_is_inside_the_bound_and_the_profile_keeps_its_promise(cid):
    case = CASE[cid]
    api, kv_t, D, N, H, Hkv, n_kv, n_past, profs, mm, ML = case
    d = FM.case_data(case)
    ref = d["ref"]
    out, info = FM.emulate_case(case)
    ratio = ratio_of(out, ref)
    print(f"emulation |got - R| / bound: {ratio.max():.3f} {cid}")
    assert np.all(np.isfinite(out)) and np.all(ratio <= 1.0), float(ratio.max())
    assert np.all(out[ref["n_vis"] == 0] == 0.0)
    # the bound is not vacuous
    live = ref["A"] > 0
    assert np.median(ref["bound"][live] / np.maximum(np.abs(ref["R"]), ref["A"] / 100)[live]) < 2.0 ** -9
    # |scaled scores| <= 60 nats, operands inside fp16
    assert np.max(np.abs(ref["x2"][np.isfinite(ref["x2"])])) <= 60 * FM.LOG2E and max(np.abs(d["Kop"]).max(), np.abs(d["Vop"]).max(), np.abs(d["Qop"]).max()) < 100
    vt = visible_tiles(case)
    decode, chunk, splits = d["plan"]
    for b, p in enumerate(profs):
        resc, big = info["rescales"][b], info["big_p"][b]
        if p == "ascending":
            assert np.all(resc >= np.maximum(vt[b] - 1, 0).sum(-1))
            if splits > 2:
                assert np.all(info["wmin"][b] < -2 * FM.FA_TAU)                  # merge weights far from 1
        elif p == "stairs7":
            two, three = vt[b].sum(-1) >= 2, vt[b].sum(-1) >= 3           # +7: p up to 2^7 against the old reference; +14: the reference moves
            assert two.any() and np.all(big[two] >= 1) and np.all(resc[three] >= 1) and (three.any() or mm == "bias")
        elif p == "descending":
            assert np.all(resc == 0)
            x = ref["x2"][b]
            with np.errstate(invalid="ignore"):
                below = x - np.max(x, axis=-1, keepdims=True)
            if n_kv >= 129:
                assert np.any((below < -14) & (below > -24)) and np.any((below < -24) & np.isfinite(below))
        elif p == "split_maxima" and splits > 1:
            assert np.all(info["wmin"][b] < -40)
        elif p == "edge":                                                         # the last visible key carries the largest weight of its row
            x = ref["x2"][b]
            last = n_kv - 1 - np.argmax(np.isfinite(x)[..., ::-1], axis=-1)
            assert np.all((np.argmax(x, axis=-1) == last) | (ref["n_vis"][b].T == 0))
    if mm == "bias":
        assert np.any(ref["n_vis"] == 0) or decode                               # a fully masked query
        assert np.any(vt == 0)                                                   # and a fully masked tile / split


def test_the_half_precision_rounding_of_p_leads_at_ordinary_score_magnitudes():
    """Gaussian q and k (the data of tests/test_gpu_fattn.py): 2^-11 A is more than half of the bound at the median element, at both head sizes, decode and prefill"""
    for D, N, H, Hkv, n_kv, n_past, mm in [(128, 1, 8, 2, 300, 299, "causal"), (64, 130, 4, 2, 191, 61, "causal"), (128, 130, 4, 2, 191, 61, "bias")]:
        for kv_t in (FM.F16, FM.Q8_0):
            q, k, v, mask = FM.profile("gaussian", D, N, H, Hkv, n_kv, n_past, kv_t, 0, mm)
            plan = FM.launch_plan(N, H, Hkv, n_kv)
            ref = FM.reference(FM.q_operand(kv_t, q)[None], FM.kv_operand(kv_t, k)[None], FM.kv_operand(kv_t, v)[None], mask, None, 1 / np.sqrt(D), n_kv, plan)
            live = ref["A"] > 0
            assert np.median(FM.U16 * ref["A"][live] / ref["bound"][live]) > 0.5


# ---- a wrong kernel fails ----------------------------------------------------------------------------------------------------------
def _rescaled(case, info, ref):
    return info["rescales"] >= 1


def _all(case, info, ref):
    return ref["n_vis"] > 0


def _not_last_query(case, info, ref):
    t = ref["n_vis"] > 0
    t[:, -1] = False
    return t


def _group_edge_heads(case, info, ref):
    H, r = case[4], case[4] // case[5]
    t = np.zeros(ref["n_vis"].shape, bool)
    t[:, :, [h for h in range(H) if ((h + 1) % H) // r != h // r]] = True
    return t


def _batch_1(case, info, ref):
    t = np.zeros(ref["n_vis"].shape, bool)
    t[1] = True
    return t


# (mutation, the case(s) it is shown on -- profile named in the case id, the rows it touches)
MUTANTS = [
    ("no_l_rescale", ["fa-1-128-130-4-2-191-61-ascending-causal-0", "fa-8-64-130-4-2-191-61-stairs7-causal-0", "prefill-1-128-200-4-2-261-61-ascending-None-280"], _rescaled),
    ("no_o_rescale", ["fa-1-128-130-4-2-191-61-ascending-causal-0", "fa-8-64-130-4-2-191-61-stairs7-causal-0", "prefill-1-128-200-4-2-261-61-ascending-None-280"], _rescaled),
    ("lim_plus", ["prefill-1-128-130-4-2-191-61-edge-None-208", "prefill-1-64-130-4-2-191-61-edge-None-208"], _not_last_query),
    ("lim_minus", ["prefill-1-128-130-4-2-191-61-edge-None-208", "prefill-1-128-130-4-2-130-0-edge-None-152"], _all),
    ("drop_last_ragged", ["fa-1-128-1-8-2-300-299-ascending-None-0", "fa-1-128-1-8-2-65-64-ascending-None-0"], _all),
    ("leak_hidden", ["fa-1-128-11-6-2-81-70-edge-causal-0", "fa-8-128-8-8-2-78-70-edge-causal-0"], _not_last_query),
    ("leak_hidden", ["prefill-1-128-200-4-2-261-61-edge-None-280"], _all),                                          # the last query reads the cache row past n_kv
    ("merge_w1", ["fa-1-128-1-8-2-300-299-split_maxima-None-0", "fa-8-128-1-8-2-300-299-ascending-bias-0", "fa-1-64-1-4-4-8128-8127-split_maxima-None-0"], _all),
    ("merge_l_unweighted", ["fa-1-128-1-8-2-300-299-split_maxima-bias-0", "fa-1-128-1-8-2-300-299-ascending-None-0", "fa-1-64-1-4-4-8128-8127-split_maxima-None-0"], _all),
    ("mask_row_next", ["fa-1-128-11-6-2-81-70-edge-causal-0", "fa-8-128-8-8-2-78-70-edge-causal-0"], _all),
    ("kv_head_next", ["fa-8-128-1-8-2-300-299-sink_mixed-causal-0", "fa-1-128-130-4-2-191-61-edge-causal-0"], _group_edge_heads),
    ("k_batch0", ["fa-1-128-1-8-2-300-299-ascending+split_maxima-heads-0", "fa-8-64-130-4-2-191-61-edge+descending-heads-0"], _batch_1),
]


@pytest.mark.parametrize("mutation,cids,touched", MUTANTS, ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTANTS)])
def test_mutants_violate_the_bound_at_every_row_they_touch(mutation, cids, touched):
    for cid in cids:
        case = CASE[cid]
        ref = FM.case_data(case)["ref"]
        _, info = FM.emulate_case(case)
        out, _ = FM.emulate_case(case, [mutation])
        t = touched(case, info, ref)
        assert t.sum() >= 1, cid
        bad = rows_outside(out, ref)
        assert np.all(bad[t]), (cid, int(t.sum()), int((t & ~bad).sum()))


def test_every_mutation_is_covered():
    assert {m[0] for m in MUTANTS} == set(FM.MUTATIONS)


# ---- the check this bound joins would have missed it ---------------------------------------------------------------------------------
def test_the_max_norm_check_misses_mutants():
    """tests/test_gpu_fattn.py's max |got - want| / max |want| < FA_EXACT (a) cannot see a lost `l_run *= alpha` on its own Gaussian data -- no row ever rescales,
    the mutant's output is the same words -- and (b) passes a kernel that hides the last key of the ragged last tile on sink_mixed, where the rows with a sink
    (|v| 8 times the others) set max |want|; the per-element bound catches both, (a) on `ascending`"""
    rel = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b)))
    D, N, H, Hkv, n_kv, n_past = 128, 130, 4, 2, 191, 61
    q, k, v, mask = FM.profile("gaussian", D, N, H, Hkv, n_kv, n_past, FM.F16, 0, "causal")
    ops = (FM.q_operand(FM.F16, q)[None], FM.kv_operand(FM.F16, k)[None], FM.kv_operand(FM.F16, v)[None], mask, None, np.float32(1 / np.sqrt(D)), n_kv,
           FM.launch_plan(N, H, Hkv, n_kv))
    base, info = FM.emulate(*ops)
    for m in ("no_l_rescale", "no_o_rescale"):
        mut, _ = FM.emulate(*ops, mutate=[m])
        assert np.all(info["rescales"] == 0) and np.array_equal(mut, base)

    cid = "fa-1-128-1-8-2-300-299-sink_mixed-causal-0"
    ref = FM.case_data(CASE[cid])["ref"]
    mut, _ = FM.emulate_case(CASE[cid], ["drop_last_ragged"])
    assert rel(mut, ref["R"]) < FA_EXACT
    bad = rows_outside(mut, ref)[0, 0]                                        # [H]: odd heads are the diffuse ones
    assert np.all(bad[1::2]), bad
    print(f"drop_last_ragged on sink_mixed: max-norm {rel(mut, ref['R']):.2e}, |got - R| / bound up to {ratio_of(mut, ref).max():.1f}")
