"""GPU: flash attention at head sizes 96 and 256 (fattn.h: k_fattn and k_fattn_merge, as fattn_hs.hip instantiates them) element by element against float64.

Operands, float64 reference and per-element bound come from tests/fattn_model.py (the bound does not depend on D); the call and the three assertions are
those of tests/test_gpu_fattn_bounds.py.  The cases are the smallest shapes that reach each path: decode with packed GQA rows, 5 splits and a 44-position
tail; a second split of one key; N r = 32 (the last decode shape) and 33 (the first prefill shape, a ragged query block); two query blocks with a fully
masked leading tile, a fully masked query and repeated rescales; p > 1 under the lazy reference; a per-head mask over two batches."""
import numpy as np
import pytest

import fattn_model as FM
from test_gpu_fattn_bounds import run_flash_attn_ext

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 2, 300, 299, ("split_maxima",), "causal"),
          (1, 8, 2, 65, 64, ("ascending",), None),
          (8, 8, 2, 78, 70, ("edge",), "causal"),
          (11, 6, 2, 81, 70, ("edge",), "causal"),
          (130, 4, 2, 191, 61, ("stairs7",), "bias"),
          (130, 4, 2, 191, 61, ("sink_mixed",), "causal")]
CASES = [("fa", kv_t, D) + s + (0,) for D in (96, 256) for kv_t in (FM.F16, FM.Q8_0) for s in SHAPES]
CASES.append(("fa", FM.F16, 256, 1, 8, 2, 300, 299, ("ascending", "split_maxima"), "heads", 0))


@pytest.mark.parametrize("case", CASES, ids=FM.case_id)
def test_flash_attention_head_sizes_96_256_inside_the_bound_at_every_element(gpu, case):
    d = FM.case_data(case)
    ref = d["ref"]
    got = run_flash_attn_ext(gpu, case, d)
    assert got.shape == ref["R"].shape
    err = np.abs(got.astype(np.float64) - ref["R"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ref["bound"] > 0, err / ref["bound"], np.where(err == 0, 0.0, np.inf))
    print(f"\n|got - R| / bound: {np.nanmax(ratio):.3f} {FM.case_id(case)}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= ref["bound"]), (float(np.nanmax(ratio)), int(np.sum(~(err <= ref["bound"]))), np.argwhere(~(err <= ref["bound"]))[:4].tolist())
    assert np.all(got[ref["n_vis"] == 0] == 0.0)                              # nothing visible -> exact zeros
