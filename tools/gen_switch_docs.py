#!/usr/bin/env python3
"""INTEGRATION.md's "Switches" section from the library's own table (cllm_options_describe, i.e. chatllm.cpp_amd/csrc/options.def).
   python tools/gen_switch_docs.py            prints the section
   python tools/gen_switch_docs.py --write    replaces what stands between the two markers in INTEGRATION.md
tests/test_options.py holds the document against the first form."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "<!-- switches:begin (tools/gen_switch_docs.py) -->", "<!-- switches:end -->"


def section():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    L = entry.load_package().lib.get()
    n = L.cllm_options_describe(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.cllm_options_describe(buf, n + 1)
    out = ["| switch | read by | kind | default | accepts | otherwise | read | numerics | meaning |", "|---|---|---|---|---|---|---|---|---|"]
    for line in buf.value.decode().splitlines():
        name, scope, kind, default, accept, bad, when, numerics, _set, _value, desc = line.split("\t")
        cell = lambda s: "`" + s.replace("|", "\\|") + "`" if s else ""
        out.append(f"| `{name}` | {scope} | {kind} | {cell(default)} | {cell(accept)} | {bad if bad != 'none' else ''} | {when} | {numerics} | {desc.replace('|', '/')} |")
    return "\n".join(out)


if __name__ == "__main__":
    text = section()
    if "--write" in sys.argv[1:]:
        path = os.path.join(ROOT, "INTEGRATION.md")
        doc = open(path).read()
        a, b = doc.index(BEGIN) + len(BEGIN), doc.index(END)
        open(path, "w").write(doc[:a] + "\n" + text + "\n" + doc[b:])
    else:
        print(text)
