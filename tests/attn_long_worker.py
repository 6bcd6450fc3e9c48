"""Worker of tests/test_gpu_attn_long.py: every case of one list of attn_long_model.CASE_LISTS through cllm_op_rope_kv_attn_decode (with the table from
cllm_op_rope_table -- "boundary_nt" cases: without one, rope_cs = NULL -- and the scratch cllm_attn_decode_wsize asks for, as ops.rope_kv_attn_decode calls it) and through the node sequence it replaces
(ROPE -> SET_ROWS, CPY of the V column, ROPE(q), MUL_MAT(K, Q), SCALE + MASK + SOFT_MAX, MUL_MAT(V, P), PERMUTE + CONT: test_rope_kv_attn_decode_equals_the_node_sequence).

CLLM_ATTN_LONG_FLASH, CLLM_ATTN_LONG_3 and CLLM_ATTN_LONG are read once per process, so every setting needs a process of its own: the test starts this file as
a script with the switch in the environment (argv: list name, out.npz); the default environment calls run_cases() in-process.  The node sequence views n_kv
positions of the caches and never reads what lies past them.

Per case (key = attn_long_model.case_key): <key>.got / .want float32 [nh * hd]; .p the node sequence's probabilities [nh, n_kv]; both caches after the call and
after the node sequence as the words that differ from the case's initial caches (.gk_i / .gk_v, .gv_i / .gv_v, .wk_i / ..: flat index and uint16 value -- the
initial caches are a function of the case, so this is the whole cache, word for word)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _diff(after, before):
    a, b = after.reshape(-1).view(np.uint16), before.reshape(-1).view(np.uint16)
    i = np.flatnonzero(a != b)
    return i.astype(np.int64), a[i]


def node_sequence(pkg, hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0, fb):
    ops, T = pkg.ops, pkg.Tensor
    QD, KD, n_past = hd * nh, hd * nkv, n_kv - 1
    pos = T.from_numpy(np.array([n_past], np.int32))
    dk, dv = T.from_numpy(kc0), T.from_numpy(vc0)
    q = T.from_numpy(qkv[:QD].reshape(1, nh, hd))
    k = T.from_numpy(qkv[QD:QD + KD].reshape(1, nkv, hd))
    v = T.from_numpy(qkv[QD + KD:].reshape(1, KD))
    ops.cpy(v.transpose(), dv.view([1, KD], [2, ML * 2], offset=n_past * 2))
    kr = ops.rope_ext(k, pos, None, hd, mode, freq_base=fb, inplace=True)
    ops.set_rows(dk.view([KD, ML], [2, KD * 2]), kr.reshape(KD, 1), pos)
    qr = ops.rope_ext(q, pos, None, hd, mode, freq_base=fb, inplace=True)
    s = ops.mul_mat(dk.view([hd, n_kv, nkv], [2, KD * 2, hd * 2]), qr.permute(0, 2, 1, 3))
    p = ops.scale_mask_soft_max(s, float(np.float32(1.0) / np.sqrt(np.float32(hd))), n_past)
    c = ops.mul_mat(dv.view([n_kv, hd, nkv], [2, ML * 2, ML * hd * 2]), p)
    want = ops.cont(c.permute(0, 2, 1, 3)).numpy().reshape(QD)
    return want, p.numpy().reshape(nh, n_kv), dk.numpy(), dv.numpy()


def one_call(pkg, hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0, fb, short_ws, table=True):
    T, L, check = pkg.Tensor, pkg.lib.get(), pkg.lib.check
    pos = T.from_numpy(np.array([n_kv - 1], np.int32))
    fk, fv, dq, dst, cs = T.from_numpy(kc0), T.from_numpy(vc0), T.from_numpy(qkv), T(pkg.F32, [hd * nh]), T(pkg.F32, [hd])
    if table:
        check(L.cllm_op_rope_table(None, pos.data_ptr(), hd, fb, cs.data_ptr()), "rope_table")
    ws = L.cllm_attn_decode_wsize(n_kv, nh, ML)
    buf = T(pkg.F32, [ws // 4 + 4]) if ws else None
    check(L.cllm_op_rope_kv_attn_decode(None, dq.data_ptr(), pos.data_ptr(), cs.data_ptr() if table else None, fb, n_kv, nh, nkv, hd, mode, fk.data_ptr(), fv.data_ptr(), ML,
                                        dst.data_ptr(), buf.data_ptr() if buf else None, (ws - 1 if short_ws else ws) if buf else 0), "rope_kv_attn_decode")
    return dst.numpy().reshape(hd * nh), fk.numpy(), fv.numpy()


def run_cases(pkg, cases):
    import attn_long_model as AL
    out = {}
    for case in cases:
        kind, hd, nh, nkv, mode, ML, n_kv, extra = case
        qkv, kc0, vc0 = AL.case_inputs(case)
        key = AL.case_key(case)
        want, p, wk, wv = node_sequence(pkg, hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0, AL.FREQ_BASE)
        got, gk, gv = one_call(pkg, hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0, AL.FREQ_BASE, kind == "short_ws", table=kind != "boundary_nt")
        out[key + ".got"], out[key + ".want"], out[key + ".p"] = got, want, p
        for name, after, before in (("gk", gk, kc0), ("gv", gv, vc0), ("wk", wk, kc0), ("wv", wv, vc0)):
            out[key + f".{name}_i"], out[key + f".{name}_v"] = _diff(after, before)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_package
    import attn_long_model as AL
    pkg = load_package()
    pkg.lib.require_gpu()
    np.savez(sys.argv[2], **run_cases(pkg, AL.CASE_LISTS[sys.argv[1]]))
