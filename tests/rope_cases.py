"""The RoPE cases that tests/test_elementwise_model.py (CPU: oracle against the reference) and tests/test_gpu_rope.py (cllm_op_rope against the
reference) share.  A case is a dense float32 parent, a view of it (ne, nb in bytes, byte offset), positions, frequency factors or None, and the
op's parameters.  All inputs are finite."""
import numpy as np

HD, N_HEAD, N_KV_HEAD, N_TOK = 64, 4, 2, 5
QKV = (N_HEAD + 2 * N_KV_HEAD) * HD                 # floats per token of the fused [q | k | v] buffer (csrc/decoder.hip)
POS5 = [0, 3, 119, 1000, 4095]
# both sides of gm_sincosf's |theta| < 120 test at pair 0, a float that is no integer (2^24 + 1), the int32 range's end, negative positions
POSITIONS = [0, 1, 2, 119, 120, 121, 4095, 131071, 1 << 20, (1 << 24) + 1, (1 << 31) - 1, -1, -120, -100000]


class Case:
    def __init__(self, name, parent, ne, nb, offset, pos, ff, **params):
        self.name, self.parent, self.offset, self.ff, self.params = name, parent, offset, ff, params
        self.ne = list(ne) + [1] * (4 - len(ne))
        self.nb = list(nb)
        while len(self.nb) < 4:
            self.nb.append(self.nb[-1] * self.ne[len(self.nb) - 1])
        self.pos = np.asarray(pos, np.int32)
        parent.setflags(write=False)

    def __repr__(self):
        return self.name

    def dense_nb(self):
        return [4, 4 * self.ne[0], 4 * self.ne[0] * self.ne[1], 4 * self.ne[0] * self.ne[1] * self.ne[2]]


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _dense(name, hd, heads, pos, seed, ff=None, **params):
    parent = _rand((len(pos), heads, hd), seed)
    return Case(name, parent, [hd, heads, len(pos)], [4, 4 * hd, 4 * hd * heads], 0, pos, ff, **params)


def layout_cases():
    """the q and the k slice of the [q | k | v] rows, padded heads, ne[3] == 2"""
    qkv = _rand((N_TOK, QKV), 11)
    p = dict(n_dims=HD, mode=2, freq_base=500000.0)
    pad = _rand((N_TOK, N_HEAD, HD + 8), 12)
    two = _rand((2, N_TOK, QKV), 13)
    return [Case("q_slice", qkv, [HD, N_HEAD, N_TOK], [4, HD * 4, QKV * 4], 0, POS5, None, **p),
            Case("k_slice", qkv, [HD, N_KV_HEAD, N_TOK], [4, HD * 4, QKV * 4], N_HEAD * HD * 4, POS5, None, **p),
            Case("padded_heads", pad, [HD, N_HEAD, N_TOK], [4, (HD + 8) * 4, (HD + 8) * 4 * N_HEAD], 0, POS5, None, **p),
            Case("ne3_2", two, [HD, N_HEAD, N_TOK, 2], [4, HD * 4, QKV * 4, QKV * 4 * N_TOK], 0, POS5, None, **p)]


def n_dims_cases():
    """n_dims == hd, hd / 2 and 2 (pass-through channels from n_dims on), both modes, on the q slice; hd == n_dims == 640: 320 pairs for the 256
    threads that fill the cos / sin cache"""
    qkv = _rand((N_TOK, QKV), 21)
    out = [Case(f"mode{mode}_n_dims{nd}", qkv, [HD, N_HEAD, N_TOK], [4, HD * 4, QKV * 4], 0, POS5, None, n_dims=nd, mode=mode, freq_base=10000.0)
           for mode in (0, 2) for nd in (HD, HD // 2, 2)]
    out += [_dense(f"mode{mode}_hd640", 640, 2, [0, 5, 4095], 22, n_dims=640, mode=mode, freq_base=1e6) for mode in (0, 2)]
    return out


def parameter_cases():
    out = [_dense("positions", HD, 2, POSITIONS, 31, n_dims=HD, mode=2, freq_base=10000.0)]
    pos = [0, 1, 7, 119, 1000, 4095, 131071]
    for base in (10000.0, 500000.0, 1e6):
        for fs in (1.0, 0.25, 1.0 / 3.0):
            out.append(_dense(f"base{base:g}_scale{fs:.3g}", HD, 2, pos, 32, n_dims=HD, mode=0, freq_base=base, freq_scale=fs))
    ff = (1.0 + np.random.default_rng(33).random(HD // 2)).astype(np.float32)
    out.append(_dense("freq_factors_scale0.25", HD, 2, pos, 34, ff=ff, n_dims=HD, mode=2, freq_base=500000.0, freq_scale=0.25))
    out.append(_dense("attn_factor1.2", HD, 2, pos, 35, n_dims=HD, mode=2, freq_base=10000.0, attn_factor=1.2))
    for ext in (1.0, 0.5):
        out.append(_dense(f"yarn_ext{ext:g}", 128, 2, pos + [20000], 36, n_dims=128, mode=2, freq_base=10000.0, n_ctx_orig=4096, freq_scale=0.25,
                          ext_factor=ext, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0))
    return out


def yarn_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow):
    """(corr0, corr1) in float32 steps, as cllm_op_rope computes them (ggml_rope_yarn_corr_dims)"""
    f = np.float32

    def corr_dim(n_rot):
        return f(f(n_dims) * np.log(f(f(n_ctx_orig) / f(f(n_rot) * f(2) * f(np.pi))), dtype=f)) / f(f(2) * np.log(f(freq_base), dtype=f))
    return max(f(0), np.floor(corr_dim(beta_fast))), min(f(n_dims - 1), np.ceil(corr_dim(beta_slow)))


# ---- the device's cos / sin swept through the op -------------------------------------------------------------------------------------------
SWEEP_TOKENS = 65536
PIO4_24 = 13176795          # round(pi/4 * 2^24): with freq_scale 2^-24 the positions around it are CONSECUTIVE floats around pi/4


def sweep_cases():
    """hd == n_dims == 2, one head, mode 0, x == (1, 0) in every token, freq_scale == 2^-k: the rotation returns (cos, sin) of pos * 2^-k exactly.
    Every threshold of gm_sincosf (2^-12, pi/4, 120) is crossed from both sides, through consecutive floats where a range of 65 536 allows it;
    then the large-argument reduction up to 2^31, negative angles of every range, and random int32 positions"""
    i = np.arange(SWEEP_TOKENS, dtype=np.int64)
    big = i * 32768 + (i * 7919) % 32768            # 0 .. 2^31 - 1, every exponent of the large-argument path
    big[-1] = (1 << 31) - 1
    ranges = [("across_2^-12", 35, (1 << 23) - 32768 + i),         # 2^-12 == 2^23 * 2^-35: every second float below it, every float above
              ("across_pi/4", 24, PIO4_24 - 32768 + i),
              ("across_120", 17, 120 * (1 << 17) - 32768 + i),     # ulp(120) == 2^-17
              ("0_to_128", 9, i),                                  # all three thresholds in one coarse pass
              ("large_to_2^31", 0, big),
              ("negative_0_to_-128", 9, -i),
              ("negative_large", 0, -big - 1),
              ("random_int32", 0, np.random.default_rng(41).integers(-(1 << 31), 1 << 31, size=SWEEP_TOKENS, dtype=np.int64))]
    x = np.zeros((SWEEP_TOKENS, 1, 2), np.float32)
    x[..., 0] = 1.0
    return [Case(name, x, [2, 1, SWEEP_TOKENS], [4, 8, 8], 0, pos.astype(np.int32), None, n_dims=2, mode=0, freq_base=10000.0, freq_scale=2.0 ** -k)
            for name, k, pos in ranges]


def sweep_angles(case):
    return case.pos.astype(np.float32) * np.float32(case.params["freq_scale"])
