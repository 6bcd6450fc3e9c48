"""CPU-only: every CLLM_* switch goes through ONE validated table (chatllm.cpp_amd/csrc/options.def, parsed by options.cpp).

The environment is parsed once per process, so every case runs in a fresh child with its environment set: either tests/options_main.cpp -- the parser alone plus a main,
built here with g++ -fsanitize=address,undefined, so every parsing case is a sanitizer run as well -- or python with the real library loaded (chatllm.cpp_amd.lib).
Expected values are what the sources did BEFORE the table existed (each case names the expression it replaces): the table must not have moved a default or a rule."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "chatllm.cpp_amd", "csrc")
HOST = os.path.join(ROOT, "chatllm.cpp_amd", "host")
COLS = ("name", "scope", "kind", "default", "accept", "bad", "when", "numerics", "set", "value", "desc")
LIVE = {"CLLM_NO_MMQ", "CLLM_NO_PREFILL_FUSE", "CLLM_NO_FUSED", "CLLM_DEBUG", "CLLM_TP_FUSED_SAME_DEVICE_ANY_SIZE", "CLLM_TP_ONESHOT_SAME_DEVICE"}
NUMERICS = {"CLLM_PREFILL", "CLLM_PREFILL_ATTN", "CLLM_DECODE_FREE_ORDER", "CLLM_HIP_TP", "CLLM_MMA_MIN_COLS", "CLLM_MMQ_MIN_COLS", "CLLM_FLASH_PREFILL", "CLLM_ATTN_LONG_FLASH"}
PYTHON_ONLY = {"CLLM_LIB", "CLLM_BENCH_TP_SELFTEST", "CLLM_BENCH_TORCH_ALLREDUCE", "CLLM_TP_ONESHOT", "CLLM_TP_FUSED", "CLLM_SKIP_BIG", "CLLM_SKIP_CFG3", "CLLM_FULL_DEPTH"}
# What an unset switch meant in the sources before the table (the literal of each `getenv(X) ? ... : <default>`; presence switches: off), as cllm_options_describe prints it
DEFAULTS = {
    "CLLM_PREFILL": "exact", "CLLM_PREFILL_ATTN": "", "CLLM_MMQ_MIN_COLS": "33", "CLLM_MMX_MIN_COLS": "-1", "CLLM_MMA_MIN_COLS": "33", "CLLM_MMF_EXACT_MIN_COLS": "2",
    "CLLM_FLASH_PREFILL": "1", "CLLM_NO_MMQ": "off", "CLLM_NO_PREFILL_FUSE": "off", "CLLM_MMD_TILE": "0", "CLLM_MMF_ZFIRST": "1", "CLLM_MMF_KQ": "1", "CLLM_MMF_PM": "0",
    "CLLM_DECODE_FREE_ORDER": "0", "CLLM_DECODE_FOLD": "1", "CLLM_NO_FUSED": "off", "CLLM_DEBUG": "off", "CLLM_GEMV_ROWS": "1", "CLLM_GEMV_ROWS32": "1", "CLLM_GEMV_TEAM32": "1",
    "CLLM_MMVQ_WG": "256", "CLLM_MMVQ_OCC": "8", "CLLM_ATTN_LONG": "512", "CLLM_ATTN_LONG_3": "0", "CLLM_ATTN_LONG_FLASH": "0", "CLLM_FA_DIV": "64",
    "CLLM_TP_ONESHOT_SAME_DEVICE": "", "CLLM_TP_FUSED_SAME_DEVICE_ANY_SIZE": "off",
    "CLLM_HIP_TP": "0", "CLLM_HIP_VIRTUAL_DEVICES": "0", "CLLM_HIP_TP_STREAMS": "0", "CLLM_HIP_TP_HEAD": "1", "CLLM_HIP_TP_GRAPH": "1", "CLLM_HIP_TP_DEBUG": "off", "CLLM_HIP_GRAPH": "1",
    "CLLM_HIP_NO_FUSE": "off", "CLLM_HIP_NO_PREFILL_FUSE": "off", "CLLM_HIP_NO_MOE_DOWN_FUSE": "off", "CLLM_HIP_MOE_FOLD": "1", "CLLM_HIP_FUSE_ATTN": "2", "CLLM_HIP_FORCE_STAGE": "off",
    "CLLM_HIP_PACK": "1", "CLLM_HIP_PACK_GB": "-1", "CLLM_HIP_SYNC_LOAD": "off", "CLLM_HIP_AHEAD": "1", "CLLM_HIP_AHEAD_CHAIN": "1", "CLLM_HIP_AHEAD_ONE": "1", "CLLM_HIP_AHEAD_LATE": "off",
    "CLLM_HIP_AHEAD_SYNC": "off", "CLLM_HIP_AHEAD_TIMING": "off", "CLLM_HIP_AHEAD_DEBUG": "off", "CLLM_HIP_STATS": "off", "CLLM_HIP_TRACE": "off", "CLLM_HIP_SIG_DEBUG": "off",
}


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CLLM_")}
    env.update(extra)
    return env


def table(text):
    rows = [dict(zip(COLS, line.split("\t"))) for line in text.splitlines()]
    assert all(len(r) == len(COLS) for r in rows), text[:300]
    return {r["name"]: r for r in rows}


@pytest.fixture(scope="session")
def parser_exe(tmp_path_factory):
    """the parser's translation unit + tests/options_main.cpp, nothing else, under AddressSanitizer and UBSan (any finding aborts: the run's exit status says so)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the parser alone"
    exe = str(tmp_path_factory.mktemp("options") / "options_main")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                        os.path.join(CSRC, "options.cpp"), os.path.join(ROOT, "tests", "options_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_parser(exe, env):
    r = subprocess.run([exe], env=dict(env, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return table(r.stdout), r.stderr.splitlines()


def run_library(code, **extra):
    """python with the real library loaded; `code` sees L (the ctypes library), describe() (the table as a dict) and os"""
    head = ("import ctypes, json, os, sys\n"
            f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "from conftest import load_package\n"
            "L = load_package().lib.get()\n"
            "def describe():\n"
            "    n = L.cllm_options_describe(None, 0); b = ctypes.create_string_buffer(n + 1); assert L.cllm_options_describe(b, n + 1) == n\n"
            "    return b.value.decode()\n")
    r = subprocess.run([sys.executable, "-c", head + code], env=clean_env(**extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout, r.stderr.splitlines()


# ---- 1. the sources ----------------------------------------------------------------------------------------------------------------------------------
def _sources(d):
    return {f: open(os.path.join(d, f), errors="ignore").read() for f in sorted(os.listdir(d)) if f.endswith((".hip", ".h", ".cpp"))}


def _def_rows():
    txt = open(os.path.join(CSRC, "options.def")).read()
    rows = re.findall(r"^CLLM_OPTION\((CLLM_\w+),\s*(\w+),\s*(\w+),.*?,\s*(latched|live),\s*(yes|no),", txt, re.M)
    assert len(rows) == txt.count("\nCLLM_OPTION(")
    return {name: dict(scope=scope, kind=kind, when=when, numerics=num) for name, scope, kind, when, num in rows}


def test_only_the_parser_reads_the_environment_and_every_row_is_used():
    rows = _def_rows()
    lib_src, host_src = _sources(CSRC), _sources(HOST)
    for f, txt in list(lib_src.items()) + list(host_src.items()):
        if f != "options.cpp":
            assert "getenv" not in txt, f
    assert lib_src["options.cpp"].count("getenv(") >= 1
    used_lib = set()
    for f, txt in lib_src.items():
        if f.endswith(".hip") or f == "common.h":
            used_lib |= set(re.findall(r"\bOPT_(CLLM_\w+)", txt))
    used_host = set()
    for txt in host_src.values():
        used_host |= set(re.findall(r'cllm_option_\w+\(\s*"(\w+)"', txt))
    assert used_lib and used_host
    assert not (used_lib | used_host) - set(rows), sorted((used_lib | used_host) - set(rows))            # every name a call site asks for is registered
    assert used_lib == {n for n, r in rows.items() if r["scope"] == "lib"}                                  # ... by its own side, and no row is dead
    assert used_host == {n for n, r in rows.items() if r["scope"] == "host"}
    assert {n for n, r in rows.items() if r["scope"] == "python"} == PYTHON_ONLY
    assert {n for n, r in rows.items() if r["when"] == "live"} == LIVE
    assert {n for n, r in rows.items() if r["numerics"] == "yes"} == NUMERICS
    assert set(DEFAULTS) == {n for n, r in rows.items() if r["scope"] != "python"} and len(DEFAULTS) == 54
    # the parser stands alone: no HIP, no other header of the library
    assert re.findall(r'#include\s+[<"]([^>"]+)', lib_src["options.cpp"] + lib_src["options.h"]).count("options.h") == 1
    assert not re.search(r"#include\s+[<\"](hip|common)", lib_src["options.cpp"] + lib_src["options.h"])


# ---- 2. defaults -------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_set_means_the_old_defaults_and_silence(parser_exe):
    out, err = run_library("print(describe())\n"
                           "print(json.dumps([L.cllm_get_prefill_mode(), L.cllm_get_decode_free_order(), L.cllm_attn_prefill_min_cols(), L.cllm_mul_mat_ex_min_cols()]))\n")
    assert err == []
    body, modes = out.strip().rsplit("\n", 1)
    t = table(body.strip("\n"))
    assert {n: r["value"] for n, r in t.items() if r["scope"] != "python"} == DEFAULTS
    assert all(r["set"] == "0" for r in t.values()) and all(t[n]["value"] == "" for n in PYTHON_ONLY)
    assert {n: r["default"] for n, r in t.items() if r["kind"] != "presence" and r["scope"] != "python"} == {n: v for n, v in DEFAULTS.items() if v not in ("on", "off")}
    assert {n for n, r in t.items() if r["when"] == "live"} == LIVE and {n for n, r in t.items() if r["numerics"] == "yes"} == NUMERICS
    assert modes == "[1, 0, 33, 10]"          # exact prefill, exact decode order, the flash form from 33 query rows, the exact-order GEMM from 10 columns (no CLLM_MMX_MIN_COLS, a narrow shape)
    t2, err2 = run_parser(parser_exe, clean_env())                # the stand-alone parser is the same table
    assert err2 == [] and t2 == t


# ---- 3. parsing: (environment, switch, value used, what the warning must contain or None) -- each against the expression the table replaced ------------------
PARSE = [
    # capi.hip: e && (!strcmp(e, "fast") || !strcmp(e, "f16")) ? fast : exact; dense_f16.hip: e && !strcmp(e, "f16")
    ({"CLLM_PREFILL": "fast"}, "CLLM_PREFILL", "fast", None), ({"CLLM_PREFILL": "f16"}, "CLLM_PREFILL", "f16", None), ({"CLLM_PREFILL": "exact"}, "CLLM_PREFILL", "exact", None),
    ({"CLLM_PREFILL": "F16"}, "CLLM_PREFILL", "exact", "CLLM_PREFILL=F16 is not one of exact|fast|f16"), ({"CLLM_PREFILL": ""}, "CLLM_PREFILL", "exact", "CLLM_PREFILL= is not one of"),
    ({"CLLM_HIP_NO_FUSE": "0"}, "CLLM_HIP_NO_FUSE", "on", "is a presence switch: any value, including 0, turns it on; unset it instead"),      # getenv(X) != nullptr
    ({"CLLM_HIP_GRAPH": "0"}, "CLLM_HIP_GRAPH", "0", None), ({"CLLM_HIP_GRAPH": "1"}, "CLLM_HIP_GRAPH", "1", None),                        # off iff atoi == 0
    ({"CLLM_HIP_FUSE_ATTN": "0"}, "CLLM_HIP_FUSE_ATTN", "0", None), ({"CLLM_HIP_FUSE_ATTN": "1"}, "CLLM_HIP_FUSE_ATTN", "1", None), ({"CLLM_HIP_FUSE_ATTN": "2"}, "CLLM_HIP_FUSE_ATTN", "2", None),
    # mmvq.hip: v == 64 || 128 || 256 || 512 || 1024, else the 256 it was initialised with
    ({"CLLM_MMVQ_WG": "64"}, "CLLM_MMVQ_WG", "64", None), ({"CLLM_MMVQ_WG": "1024"}, "CLLM_MMVQ_WG", "1024", None), ({"CLLM_MMVQ_WG": "100"}, "CLLM_MMVQ_WG", "256", "CLLM_MMVQ_WG=100"),
    # mmvq.hip: v >= 1 && v <= 32, else the 8 it was initialised with
    ({"CLLM_MMVQ_OCC": "0"}, "CLLM_MMVQ_OCC", "8", "CLLM_MMVQ_OCC=0"), ({"CLLM_MMVQ_OCC": "1"}, "CLLM_MMVQ_OCC", "1", None), ({"CLLM_MMVQ_OCC": "32"}, "CLLM_MMVQ_OCC", "32", None),
    ({"CLLM_MMVQ_OCC": "33"}, "CLLM_MMVQ_OCC", "8", "CLLM_MMVQ_OCC=33"),
    # decoder.hip: v < 64 ? 64 : v
    ({"CLLM_ATTN_LONG": "32"}, "CLLM_ATTN_LONG", "64", "CLLM_ATTN_LONG=32"), ({"CLLM_ATTN_LONG": "64"}, "CLLM_ATTN_LONG", "64", None), ({"CLLM_ATTN_LONG": "4096"}, "CLLM_ATTN_LONG", "4096", None),
    # gemv_free32.hip: atoi > 0 ? 1 : 0
    ({"CLLM_DECODE_FREE_ORDER": "0"}, "CLLM_DECODE_FREE_ORDER", "0", None), ({"CLLM_DECODE_FREE_ORDER": "1"}, "CLLM_DECODE_FREE_ORDER", "1", None),
    ({"CLLM_DECODE_FREE_ORDER": "2"}, "CLLM_DECODE_FREE_ORDER", "1", "CLLM_DECODE_FREE_ORDER=2"), ({"CLLM_DECODE_FREE_ORDER": "-1"}, "CLLM_DECODE_FREE_ORDER", "0", "CLLM_DECODE_FREE_ORDER=-1"),
    # ggml-hip.cpp: k > 1 ? min(k, 16) : ignored (the call site still asks for > 1: a 1 is accepted and means off)
    ({"CLLM_HIP_TP": "1"}, "CLLM_HIP_TP", "1", None), ({"CLLM_HIP_TP": "2"}, "CLLM_HIP_TP", "2", None), ({"CLLM_HIP_TP": "16"}, "CLLM_HIP_TP", "16", None),
    ({"CLLM_HIP_TP": "17"}, "CLLM_HIP_TP", "16", "CLLM_HIP_TP=17"),
    # ggml-hip.cpp: k > 0 ? min(k, 64) : ignored
    ({"CLLM_HIP_VIRTUAL_DEVICES": "0"}, "CLLM_HIP_VIRTUAL_DEVICES", "0", None), ({"CLLM_HIP_VIRTUAL_DEVICES": "65"}, "CLLM_HIP_VIRTUAL_DEVICES", "64", "CLLM_HIP_VIRTUAL_DEVICES=65"),
    ({"CLLM_HIP_PACK_GB": "1.5"}, "CLLM_HIP_PACK_GB", "1.5", None), ({}, "CLLM_HIP_PACK_GB", "-1", None),                                 # atof, else -1.0
    # matmul_f.hip's reading, which fattn.hip now shares: any number is taken, something that is not a number is the default
    ({"CLLM_MMA_MIN_COLS": "8"}, "CLLM_MMA_MIN_COLS", "8", None), ({"CLLM_MMA_MIN_COLS": "many"}, "CLLM_MMA_MIN_COLS", "33", "CLLM_MMA_MIN_COLS=many is not a number"),
    # everywhere else a value that is not a number is still what atoi makes of it -- and now said
    ({"CLLM_HIP_GRAPH": "off"}, "CLLM_HIP_GRAPH", "0", "CLLM_HIP_GRAPH=off is not a number"),
]


@pytest.mark.parametrize("env,name,value,warning", PARSE, ids=[f"{n}={e.get(n, '<unset>')}" for e, n, _, _ in PARSE])
def test_a_value_means_what_it_meant_before(parser_exe, env, name, value, warning):
    t, err = run_parser(parser_exe, clean_env(**env))
    assert t[name]["value"] == value and t[name]["set"] == ("1" if name in env else "0")
    warnings = [ln for ln in err if ln.startswith("[cllm] warning: ")]
    if warning is None:
        assert warnings == []
    else:
        assert len(warnings) == 1 and warning in warnings[0], err
        if t[name]["kind"] != "presence":
            assert f"{value} is used" in warnings[0] or f"read as {value}" in warnings[0], warnings[0]      # the warning says what is used instead
    notes = [ln for ln in err if ln.startswith("[cllm] note: ")]
    assert notes == ([f"[cllm] note: {name} is set and changes numerics: {value} is used"] if name in NUMERICS and name in env else [])
    assert len(err) == len(warnings) + len(notes)
    assert {n: r["value"] for n, r in t.items() if n != name and r["scope"] != "python"} == {n: v for n, v in DEFAULTS.items() if n != name}


@pytest.mark.parametrize("word,mode", [("fast", 0), ("f16", 0), ("exact", 1), ("F16", 1), ("", 1)])
def test_the_prefill_word_sets_the_mode_it_set_before(word, mode):
    """through the real library: capi.hip took fast and f16 for the fast mode and everything else -- F16 and the empty string too -- for the exact one; now with a warning"""
    out, err = run_library("print(L.cllm_get_prefill_mode(), L.cllm_option_str(b'CLLM_PREFILL').decode())\n", CLLM_PREFILL=word)
    assert out.split() == [str(mode), word if word in ("fast", "f16", "exact") else "exact"]
    assert sum(ln.startswith("[cllm] warning: CLLM_PREFILL=") for ln in err) == (0 if word in ("fast", "f16", "exact") else 1)


# ---- 4. names nobody registered ----------------------------------------------------------------------------------------------------------------------
def test_an_unknown_name_is_said_once_with_its_nearest_neighbour(parser_exe):
    t, err = run_parser(parser_exe, clean_env(CLLM_HIP_TPP="2"))
    assert len(err) == 1 and err[0].startswith("[cllm] warning: CLLM_HIP_TPP ") and err[0].endswith("did you mean CLLM_HIP_TP?")
    assert t["CLLM_HIP_TP"]["value"] == "0" and t["CLLM_HIP_TP"]["set"] == "0"
    _, err = run_parser(parser_exe, clean_env(CLLM_FULL_DEPTH="1", CLLM_LIB=os.path.join(ROOT, "chatllm.cpp_amd", "libchatllm_hip.so")))
    assert err == []
    _, err = run_parser(parser_exe, clean_env(CLLM_FFN_FUSED="1"))          # a closed experiment's switch (tools/round6): not registered on purpose
    assert len(err) == 1 and err[0].startswith("[cllm] warning: CLLM_FFN_FUSED ")
    out, err = run_library("print(describe().count('\\n'))\n", CLLM_HIP_TPP="2")         # the library says the same
    assert len(err) == 1 and err[0].endswith("did you mean CLLM_HIP_TP?") and int(out) == len(DEFAULTS) + len(PYTHON_ONLY)


# ---- 5. live and latched, and the by-name ABI's errors ---------------------------------------------------------------------------------------------------
def test_live_switches_follow_the_environment_latched_ones_do_not():
    out, err = run_library(
        "r = [L.cllm_option_is_set(b'CLLM_NO_FUSED'), L.cllm_option_int(b'CLLM_GEMV_ROWS')]\n"
        "os.environ['CLLM_NO_FUSED'] = '1'; os.environ['CLLM_GEMV_ROWS'] = '0'\n"
        "r += [L.cllm_option_is_set(b'CLLM_NO_FUSED'), L.cllm_option_int(b'CLLM_GEMV_ROWS')]\n"
        "del os.environ['CLLM_NO_FUSED']\n"
        "r += [L.cllm_option_is_set(b'CLLM_NO_FUSED')]\n"
        "r += [L.cllm_option_int(b'CLLM_NOPE'), L.cllm_last_error().decode()]\n"
        "r += [L.cllm_option_int(b'CLLM_PREFILL'), L.cllm_last_error().decode(), L.cllm_option_str(b'CLLM_GEMV_ROWS'), L.cllm_option_real(b'CLLM_HIP_PACK_GB')]\n"
        "print(json.dumps(r))\n")
    import json
    r = json.loads(out)
    assert r[:5] == [0, 1, 1, 1, 0]                      # CLLM_NO_FUSED: off, on, off again (tests/test_gpu_tp.py flips it in a live process); CLLM_GEMV_ROWS stays 1
    assert r[5] == 0 and "CLLM_NOPE is not a registered switch" in r[6]
    assert r[7] == 0 and "CLLM_PREFILL is not of that kind" in r[8] and r[9] is None and r[10] == -1.0
    assert err == []


# ---- 6. the document -----------------------------------------------------------------------------------------------------------------------------------
def test_integration_md_lists_the_table_as_the_library_prints_it():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_switch_docs.py")], env=clean_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- switches:begin[^>]*-->\n(.*?)\n<!-- switches:end -->", doc, re.S)
    assert m, "INTEGRATION.md: the Switches section's markers"
    assert m.group(1) == r.stdout.rstrip("\n"), "INTEGRATION.md is stale: python tools/gen_switch_docs.py --write"
    assert m.group(1).count("\n| `CLLM_") == len(DEFAULTS) + len(PYTHON_ONLY)


# ---- 7. what only a sanitizer sees (every case above already ran the parser under ASan + UBSan) -----------------------------------------------------------
def test_the_parser_survives_a_hostile_environment(parser_exe):
    t, err = run_parser(parser_exe, clean_env(CLLM_PREFILL="x" * 4096, CLLM_HIP_TP="9" * 4096, CLLM_HIP_NO_FUSE="0" * 4096))         # 4 KB values
    assert t["CLLM_PREFILL"]["value"] == "exact" and t["CLLM_HIP_NO_FUSE"]["value"] == "on" and all(len(ln) < 400 for ln in err)
    assert sum(ln.startswith("[cllm] warning: ") for ln in err) == 2
    t, err = run_parser(parser_exe, clean_env(**{"CLLM_": "", "CLLM_" + "Y" * 300: "1"}))                                        # an empty tail, a name longer than any buffer
    assert len(err) == 2 and sum(ln.startswith("[cllm] warning: CLLM_ is not") for ln in err) == 1
    big = clean_env(**{f"FILLER_{i}": "v" * (i % 50) for i in range(2000)}, CLLM_HIP_TPP="2", CLLM_MMVQ_WG="100")                      # 2000 entries around two findings
    t, err = run_parser(parser_exe, big)
    assert len(err) == 2 and t["CLLM_MMVQ_WG"]["value"] == "256"
