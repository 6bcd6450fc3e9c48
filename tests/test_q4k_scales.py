"""CPU-only: the Q4_K / Q5_K 6-bit scale / min unpack is stated ONCE, in chatllm.cpp_amd/csrc/q4k_scales.h (every kernel calls q4k_scales).  The header compiles
alone with g++ and equals get_scale_min_k4 written byte by byte, for all eight sub-blocks: the all-zero, all-ones and 96 single-bit headers and 10 000 random ones."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "chatllm.cpp_amd", "csrc")


def test_q4k_scales_equals_get_scale_min_k4(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the header alone"
    exe = str(tmp_path / "q4k_scales_main")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "q4k_scales_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
    assert r.stdout.split() == ["10098", "headers,", "0", "mismatches"]
    assert not re.search(r"#include\s+[<\"](hip|common)", open(os.path.join(CSRC, "q4k_scales.h")).read())


def test_the_unpack_and_the_tile_gemm_shell_are_stated_once():
    src = {f: open(os.path.join(CSRC, f), errors="ignore").read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp"))}
    assert [f for f, t in src.items() if "0x3f3f3f3f" in t] == ["q4k_scales.h"]
    assert [f for f, t in src.items() if "0x64646464" in t] == ["mm_tile.h"]
    assert [f for f, t in src.items() if re.search(r"DPP_QUAD_XOR1>\([^\n]*\n[^\n]*silu_any\(", t)] == ["mm_tile.h"]
    for f in ("mmq.hip", "mmx.hip", "dense_f16.hip"):
        assert "hipFuncAttributeMaxDynamicSharedMemorySize" not in src[f] and '#include "mm_tile.h"' in src[f], f
