"""CPU-only: what a tensor type IS is stated ONCE, in chatllm.cpp_amd/csrc/types.def (read through types.h).  (a) the sources hold no second list; (b) every row agrees with
the public enum, the Python dicts, the oracle and -- where it is built -- the reference's own type traits, which are the yardstick; (c) types.h compiles alone with g++."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "chatllm.cpp_amd", "csrc")
HOST = os.path.join(ROOT, "chatllm.cpp_amd", "host")
ACT = {"none": 0, "q8_0": 32, "q8_1": 33, "q8_k": 256}          # types.h: ACT_*
GGML_VEC_DOT = {"q8_0": 8, "q8_1": 9, "q8_k": 15}                 # enum ggml_type: GGML_TYPE_Q8_0 / Q8_1 / Q8_K


def _rows():
    txt = open(os.path.join(CSRC, "types.def")).read()
    rows = re.findall(r"^CLLM_WTYPE\((\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\w+),\s*(\w+),\s*(\d+),\s*([\w |]+)\)", txt, re.M)
    assert len(rows) == txt.count("\nCLLM_WTYPE(") == 26
    out = {}
    for name, id_, size, blck, act, fam, align, flags in rows:
        out[name] = dict(id=int(id_), size=int(size), blck=int(blck), act=act, family=fam, align=int(align), flags={f.strip() for f in flags.split("|")} - {"no_flags"})
    assert len({r["id"] for r in out.values()}) == 26
    return out


def _sources():
    src = {}
    for d in (CSRC, HOST):
        for f in sorted(os.listdir(d)):
            if f.endswith((".hip", ".h", ".cpp")) and f != "types.h":
                src[os.path.join(os.path.basename(d), f)] = open(os.path.join(d, f), errors="ignore").read()
    return src


# ---- (a) one statement only ------------------------------------------------------------------------------------------------------------------------------
def test_the_sources_hold_no_second_list_of_types():
    for f, txt in _sources().items():
        assert not re.search(r"case\s+CLLM_TYPE_\w+\s*:\s*return\s+\d", txt), f                                          # no trait switch
        assert not re.search(r"([\w>.\-]+)\s*==\s*(CLLM|GGML)_TYPE_\w+(\s*\|\|\s*\1\s*==\s*(CLLM|GGML)_TYPE_\w+){2,}", txt), f     # no || chain of three or more type comparisons of one value
        assert not re.search(r"\?\s*\d+\s*:[^;\n]*TYPE_\w+\s*\?\s*\d+\s*:", txt), f                                      # no `== X ? 66 : == Y ? 74 :` block-size chain
        assert not re.search(r"\?\s*(18|20|34|144|176|210|22|24|17|84|110|136|54|66|74|82|98|50|56)\s*:\s*(18|20|34|144|176|210|22|24|17|84|110|136|54|66|74|82|98|50|56)\b", txt), f


def test_capi_has_one_timer_and_one_call_site_per_gemm_launcher():
    src = _sources()
    capi = src[os.path.join("csrc", "capi.hip")]
    assert capi.count("hipEventElapsedTime(") == 2 and "cllm_event_elapsed_ms" in capi          # the ABI's own + timed_launches
    assert capi.count("hipEventCreate(") == 3                                                     # cllm_event_create + the timer's two
    everything = "\n".join(src.values())
    for fn in ("launch_mmx", "launch_mmq", "launch_dense_f16"):
        calls = [m for m in re.finditer(rf"(?<![\w ]int ){fn}\(", everything) if not re.match(r"int\s+$", everything[max(0, m.start() - 4):m.start()])]
        assert len(calls) == 1, (fn, len(calls))
    assert re.search(r"rc = launch_mmx\(", capi) and re.search(r"rc = launch_mmq\(", capi) and re.search(r"rc = launch_dense_f16\(", capi)


# ---- (b) every row against everything else that states it ---------------------------------------------------------------------------------------------------
def test_the_public_enum_is_the_table():
    hdr = open(os.path.join(ROOT, "include", "chatllm_hip.h")).read()
    enum = {n: int(v) for n, v in re.findall(r"\bCLLM_TYPE_(\w+)\s*=\s*(\d+)", hdr)}
    assert enum == {n: r["id"] for n, r in _rows().items()}


def test_the_python_dicts_are_the_table(pkg):
    T, rows = pkg.tensor, _rows()
    assert {getattr(T, n): r["size"] for n, r in rows.items()} == T.TYPE_SIZE
    assert {getattr(T, n): r["blck"] for n, r in rows.items()} == T.BLCK
    import synth_helpers, ref_ggml
    assert synth_helpers.TYPE_SIZE is T.TYPE_SIZE and synth_helpers.BLCK is T.BLCK
    assert ref_ggml._BLOCK == {r["id"]: (r["size"], r["blck"]) for r in rows.values()}


def test_the_oracle_agrees(orc):
    L = orc.lib()
    L.orc_type_size.restype, L.orc_type_size.argtypes = C.c_size_t, [C.c_int]
    L.orc_blck_size.restype, L.orc_blck_size.argtypes = C.c_int, [C.c_int]
    diffs = [n for n, r in _rows().items() if (L.orc_type_size(r["id"]), L.orc_blck_size(r["id"])) != (r["size"], r["blck"])]
    assert diffs == []


def test_the_reference_build_agrees():
    import ref_ggml
    if not ref_ggml.available():
        pytest.skip("oracle/_ref is not built here")

    class Traits(C.Structure):         # struct ggml_type_traits_cpu (ggml-cpu.h): from_float, vec_dot, vec_dot_type, nrows
        _fields_ = [("from_float", C.c_void_p), ("vec_dot", C.c_void_p), ("vec_dot_type", C.c_int), ("nrows", C.c_int64)]
    base, cpu = ref_ggml.libs()
    base.ggml_type_size.restype, base.ggml_type_size.argtypes = C.c_size_t, [C.c_int]
    base.ggml_blck_size.restype, base.ggml_blck_size.argtypes = C.c_int64, [C.c_int]
    cpu.ggml_get_type_traits_cpu.restype, cpu.ggml_get_type_traits_cpu.argtypes = C.POINTER(Traits), [C.c_int]
    diffs = []
    for n, r in _rows().items():
        if (base.ggml_type_size(r["id"]), base.ggml_blck_size(r["id"])) != (r["size"], r["blck"]):
            diffs.append((n, "size"))
        if r["act"] != "none" and cpu.ggml_get_type_traits_cpu(r["id"]).contents.vec_dot_type != GGML_VEC_DOT[r["act"]]:
            diffs.append((n, "act_kind"))
        if (r["act"] == "none") != (r["family"] == "plain"):
            diffs.append((n, "family"))
    assert diffs == []


# ---- (c) types.h alone ------------------------------------------------------------------------------------------------------------------------------------------
def test_types_h_compiles_alone_and_generates_the_table(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the header alone"
    exe = str(tmp_path / "types_main")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "types_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)                        # (the ladders: each family's rows and nothing else)
    rows = _rows()
    want = [f"{n} {r['id']} {r['size']} {r['blck']} {ACT[r['act']]} {r['align']} {int(r['family'] == 'tuned')} {int(r['family'] in ('kq256', 'kq32'))} "
            f"{int(r['blck'] == 256)} {int('iq_grid' in r['flags'])} {int('get_rows' in r['flags'])}" for n, r in rows.items()]
    assert r.stdout.splitlines() == want
    hdr = open(os.path.join(CSRC, "types.h")).read()
    assert not re.search(r"#include\s+[<\"](hip|common)", hdr)
    # the table's own sense: block sizes by family, alignments a power of two, the coverage families split by block size
    for n, r in rows.items():
        assert r["blck"] == {"plain": 1, "kq256": 256, "kq32": 32}.get(r["family"], r["blck"]) and r["align"] & (r["align"] - 1) == 0, n
    assert sorted(n for n, r in rows.items() if r["family"] == "tuned") == ["Q4_0", "Q4_1", "Q4_K", "Q8_0"]
