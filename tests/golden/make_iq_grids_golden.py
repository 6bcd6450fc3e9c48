#!/usr/bin/env python3
"""Golden tables for tests/test_golden.py::test_packed_codebooks_decode_to_the_reference_grids: the reference's IQ1 / IQ2 / IQ3
codebooks and the IQ2 sign table (ggml/src/ggml-common.h:528-1615), read as data and stored entry for entry, so that the test needs nothing
outside this repository.  The .npz is committed.
    python tests/golden/make_iq_grids_golden.py REFERENCE_SOURCE_DIR
"""
import os
import re
import sys

import numpy as np

NAMES = ("iq2xxs_grid", "iq2xs_grid", "iq2s_grid", "iq3xxs_grid", "iq3s_grid", "iq1s_grid", "ksigns_iq2xs")

src = open(os.path.join(sys.argv[1], "ggml", "src", "ggml-common.h")).read()
out = {}
for name in NAMES:
    body = re.search(r"GGML_TABLE_BEGIN\(\w+, %s, \w+\)(.*?)GGML_TABLE_END" % name, src, re.S).group(1)
    vals = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", body)] or [int(x) for x in re.findall(r"\d+", body)]
    out[name] = np.array(vals, np.uint64)
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "iq_grids_reference.npz"), **out)
print("iq_grids_reference.npz:", {k: v.shape for k, v in out.items()})
