"""GPU: flash attention at head size 112 (fattn.h: k_fattn with a padded feature block in the P.V product, k_fattn_merge with a remainder group) element by
element against float64.

112 is the first head size that is no multiple of 32: the V^T tile's last 32-row block is 16 real rows and 16 rows nobody writes, the K chunks do not divide
over the threads, the epilogue leaves stores out.  Operands, float64 reference and per-element bound come from tests/fattn_model.py (the bound does not
depend on D); the call and the three assertions are those of tests/test_gpu_fattn_head_sizes.py, and so are the shapes: decode with packed GQA rows, 5 splits
and a 44-position tail; a second split of one key; N r = 32 and 33; two query blocks with a fully masked leading tile and a fully masked query; p > 1 under
the lazy reference; a per-head mask over two batches.  F16 rows only: the host gives this head size no other cache."""
import numpy as np
import pytest

import fattn_model as FM
from test_gpu_fattn_bounds import run_flash_attn_ext
from test_gpu_fattn_head_sizes import SHAPES

pytestmark = pytest.mark.gpu

CASES = [("fa", FM.F16, 112) + s + (0,) for s in SHAPES]
CASES.append(("fa", FM.F16, 112, 1, 8, 2, 300, 299, ("ascending", "split_maxima"), "heads", 0))


@pytest.mark.parametrize("case", CASES, ids=FM.case_id)
def test_flash_attention_head_size_112_inside_the_bound_at_every_element(gpu, case):
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
