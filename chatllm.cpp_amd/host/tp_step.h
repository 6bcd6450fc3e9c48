// tp_step.h -- tensor parallel behind the ggml boundary (CLLM_HIP_TP=N): the ranks' state and one sharded decode step.
// Part of ggml-hip.cpp's translation unit: included there, inside its anonymous namespace, after the fusion planner
// (fuse_plan.h) and decode-ahead's ahead_resolve.  tp_graph_compute reads top to bottom as its steps; every step is a
// function over one tp_step, so what a step reads and writes is what it touches of that struct and of g_tp.
#pragma once

struct tp_piece { const void * src; size_t spitch, width, rows, doff, dpitch; };
struct tp_shard { void * data = nullptr; size_t bytes = 0; int n = 0; const void * src[3] = {}; uint64_t uid[3] = {}, gen[3] = {}; };
struct tp_rank {
    int gpu = 0; void * stream = nullptr; bool own_stream = false; void * fused = nullptr, * ev = nullptr;
    char * scratch = nullptr; size_t scratch_bytes = 0;
    std::unordered_map<const void *, tp_shard> shards;                   // keyed by the first source tensor's data pointer (a weight tensor has one role)
    std::vector<const void *> kv_sig; std::vector<void *> kv_mem; void * kv_table = nullptr; int64_t kv_valid = 0; uint64_t kv_epoch = 0; size_t kv_dims[3] = {};
};
// what stands in front of the sharded launches (tp_hand_over): the embedding gather's operands, where the position lives, every rank's inputs
struct tp_hand_over_args { cllm_tensor ea, eb, ed; const void * pos_src = nullptr; size_t hbytes = 0; std::vector<void *> xa, pos; };
struct tp_group {
    int n = 0; std::vector<tp_rank> r; bool fused_ready = false, broken = false, told = false, last_tp = false; int sites = 0; size_t max_n = 0; void * ev0 = nullptr;
    long steps = 0, plain = 0, replays = 0, captures = 0; const void * owner = nullptr;      // owner: the backend context whose stream rank 0 runs on
    // what a step started AHEAD of the host needs besides the captured graphs (tp_ahead_replay): the hand-over's arguments, the streams the graphs were captured on
    struct { tp_hand_over_args in; std::vector<void *> streams; std::vector<int> sgpu; int64_t n_kv = 0; bool valid = false; } rp;
    std::vector<uint64_t> last_sig, graph_sig; std::vector<void *> execs; bool graph_broken = false;      // launch-list replay of the sharded step: one captured graph per distinct stream
} g_tp;

// ---- tensor parallel BEHIND the boundary (CLLM_HIP_TP=N): ONE logical ggml device over N ranks ---------------------------------------------------------------
// The reference's own slot for this is SplitMethod::Row -- "TODO: WIP" (src/backend.h:322-327; device assignment src/backend.cpp:677-778 only splits by layer, which at
// batch 1 buys capacity, not speed).  Here the unmodified host sees a single device "HIP0"; its buffers -- weights, KV caches, activations -- live in rank 0's HBM exactly as
// on one GPU, and every graph that is not a recognised decode step (prompts, anything unusual) runs there un-sharded, bit-identical to the single-device module.  A graph that IS
// the five-launch-per-layer decode step (GET_ROWS, then per layer q|k|v -> attention -> o + residual -> gate/up -> down + residual, then norm + lm_head: the same patterns
// make_plan fuses) runs tensor-parallel:
//   * shards are cut ON THE DEVICE from the tensors the host uploaded, the first time a step needs them (like the packed copies above; validity = the source buffers' generation
//     counters): q / k / v and gate / up by ROWS (whole KV groups; F by the down projection's quant blocks, cllm_tp_split, uneven allowed), o / down by whole quant blocks of K;
//   * every rank keeps the residual stream itself; o / down send their partial rows as granules into every rank's receive buffer and the next RMS_NORM mat-vec adds them in rank
//     order (cllm_op_mul_mat_vec_tp_scatter / _gather: NO all-reduce launch, five launches per layer and rank as on one GPU); the lm_head runs on rank 0 into the host's logits;
//   * one KV shard per rank (dense, the rank's KV heads only), refreshed from the host's cache after any un-sharded graph or buffer write, and written back row by row after
//     every step (cllm_op_kv_shard_copy), so the host's cache stays what the reference expects.
// Ranks on distinct GPUs run on their own streams (the gathers poll for the peers' granules); ranks that share a GPU (N > GPUs: the one-GPU test vehicle) share rank 0's stream and
// are issued site by site, so a gather never waits for a launch that cannot start.  Everything joins rank 0's stream at the end of the step: synchronize() is unchanged.
// Results: the fp32 sums of o / down are split into N partial chains -> tolerance tier (SURVEY 8e "T1/T2"), NOT the bit-exact tier of the single device.
struct tp_layer { int gq = -1, attn = -1, o = -1, ggu = -1, down = -1; };
struct tp_desc { int embed = -1, head = -1, head_norm = -1, head_mm = -1; std::vector<tp_layer> layers; };      // head: a fused norm + mat-vec (mvs entry), or the two nodes

// is this graph the decode step the tensor-parallel path takes?  (node order: GET_ROWS, L x { q|k|v group, attention level 2, o + residual, gate/up group, down + residual }, head)
bool tp_extract(ggml_cgraph * g, const fuse_plan & P, tp_desc & D) {
    enum { S_EMBED, S_QKV, S_ATTN, S_O, S_GU, S_DOWN, S_HEAD_MM, S_DONE } st = S_EMBED;
    std::vector<uint8_t> seen(P.groups.size(), 0);
    tp_layer cur;
    for (int i = 0; i < ggml_graph_n_nodes(g); i++) {
        const ggml_tensor * t = ggml_graph_node(g, i);
        if (ggml_is_empty(t) || P.skip[i]) continue;
        if (t->op == GGML_OP_NONE || t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_PERMUTE || t->op == GGML_OP_TRANSPOSE) continue;
        if (t->op == GGML_OP_GET_ROWS) { if (st != S_EMBED) return false; D.embed = i; st = S_QKV; continue; }
        // the head as chatllm builds it (LMFinalSteps, src/models.cpp:1736-1784): the normalised hidden state is a graph OUTPUT, so the norm stays a launch of its own
        if (t->op == GGML_OP_MUL && P.alt[i] == ALT_RMS_NORM_MUL && st == S_QKV && !D.layers.empty()) { D.head_norm = i; st = S_HEAD_MM; continue; }
        if (t->op == GGML_OP_MUL_MAT && st == S_HEAD_MM && P.mv[i] < 0 && P.pf[i] < 0 && P.alt[i] == ALT_NONE) {
            const ggml_tensor * hn = ggml_graph_node(g, D.head_norm);
            if (!t->src[1] || t->src[1]->data != hn->data || ggml_nelements(t->src[1]) != hn->ne[0] || !f32_vec(t) || !is_q(t->src[0]->type)) return false;
            D.head_mm = i; st = S_DONE; continue;
        }
        if (t->op == GGML_OP_MUL_MAT && P.mv[i] >= 0 && P.alt[i] == ALT_NONE) {
            const fused_mv & f = P.mvs[P.mv[i]];
            if (f.group >= 0) {
                if (seen[f.group]) continue;                  // a later member of a group already taken
                seen[f.group] = 1;
                const merge_group & G = P.groups[f.group];
                if (!G.interleave && G.n == 3 && st == S_QKV) { cur = tp_layer(); cur.gq = f.group; st = S_ATTN; continue; }
                if (G.interleave && G.n == 2 && st == S_GU) { cur.ggu = f.group; st = S_DOWN; continue; }
                return false;
            }
            if (f.pro == 2 && f.resid && st == S_O) { cur.o = P.mv[i]; st = S_GU; continue; }
            if (f.pro == 4 && f.resid && st == S_DOWN && P.groups[cur.ggu].consumer == P.mv[i]) { cur.down = P.mv[i]; D.layers.push_back(cur); st = S_QKV; continue; }
            if (f.pro == 1 && !f.resid && st == S_QKV && !D.layers.empty()) { D.head = P.mv[i]; st = S_DONE; continue; }
            return false;
        }
        if ((t->op == GGML_OP_CPY || t->op == GGML_OP_DUP || t->op == GGML_OP_CONT) && P.attn[i] >= 0 && st == S_ATTN && P.attns[P.attn[i]].level == 2) { cur.attn = P.attn[i]; st = S_O; continue; }
        return false;
    }
    return st == S_DONE;
}

struct tp_dims { int64_t H = 0, F = 0, hd = 0; int nh = 0, nkv = 0, gs = 0; int64_t ML = 0; };
struct tp_split { int64_t kv0 = 0, kvc = 0, f0 = 0, fc = 0; };        // this rank's KV heads [kv0, kv0 + kvc) and FFN features [f0, f0 + fc)

#define FAIL_TP(msg) do { HIPB_LOG("tensor parallel: %s", msg); return CLLM_E_UNSUPPORTED; } while (0)
int tp_ensure_group(hip_backend_ctx * c, int n_sites, size_t max_n) {
    auto & T = g_tp;
    if (!T.r.empty() && T.owner != c) FAIL_TP("another backend context of this process owns the tensor-parallel ranks");
    if (T.r.empty()) {
        T.owner = c;
        const int phys = cllm_device_count();
        T.r.resize(T.n);
        for (int k = 0; k < T.n; k++) {
            tp_rank & R = T.r[k];
            R.gpu = (c->device + k) % (phys > 0 ? phys : 1);
            // CLLM_HIP_TP_STREAMS=1 (tests): ranks that share rank 0's GPU get streams of their own as well -- the event / cross-stream path of distinct GPUs on a one-GPU box.
            // Only for shapes whose launches can all be resident at once (a gather polls for scatters of other streams): the test shapes; bounded waits otherwise report a time-out.
            if (R.gpu == c->device && !(g_opt.tp_streams && k > 0)) R.stream = c->stream;
            else {
                cllm_set_device(R.gpu);
                if (int rc = cllm_stream_create(&R.stream)) { cllm_set_device(c->device); return rc; }
                if (int rc = cllm_event_create(&R.ev)) { cllm_set_device(c->device); return rc; }
                R.own_stream = true;
            }
        }
        cllm_set_device(c->device);
        if (int rc = cllm_event_create(&T.ev0)) return rc;
    }
    if (T.fused_ready && (T.sites < n_sites || T.max_n < max_n)) {              // another model on the same logical device: bigger buffers
        for (tp_rank & R : T.r) { cllm_set_device(R.gpu); cllm_stream_sync(R.stream); if (R.fused) cllm_tp_fused_destroy(R.fused); R.fused = nullptr; }
        cllm_set_device(c->device);
        T.fused_ready = false;
    }
    if (!T.fused_ready) {
        std::vector<int> devs(T.n); std::vector<void *> os(T.n, nullptr);
        for (int k = 0; k < T.n; k++) devs[k] = T.r[k].gpu;
        const size_t mn = (max_n + 3) & ~(size_t) 3;
        if (int rc = cllm_tp_fused_create_group(T.n, devs.data(), n_sites, mn, os.data())) return rc;
        for (int k = 0; k < T.n; k++) T.r[k].fused = os[k];
        T.sites = n_sites; T.max_n = mn; T.fused_ready = true;
    }
    return CLLM_OK;
}

// rank k's shard made of 2-D pieces of up to three source tensors; built on rank 0's GPU (where the sources live), moved to the rank's GPU if that is another one
void * tp_get_shard(hip_backend_ctx * c, int k, const ggml_tensor * const * srcs, int n, const tp_piece * pieces, int np, size_t bytes, bool * built) {
    tp_rank & R = g_tp.r[k];
    for (int i = 0; i < n; i++) if (!ours(srcs[i]) || ((const hip_buffer_ctx *) srcs[i]->buffer->context)->device != c->device) return nullptr;
    tp_shard & e = R.shards[srcs[0]->data];
    bool valid = e.data && e.n == n && e.bytes == bytes;
    for (int i = 0; i < n && valid; i++) { const auto * bc = (const hip_buffer_ctx *) srcs[i]->buffer->context; valid = e.src[i] == srcs[i]->data && e.uid[i] == bc->uid && e.gen[i] == bc->gen.load(); }
    if (valid) return e.data;
    if (e.data) { cllm_set_device(R.gpu); cllm_stream_sync(R.stream); cllm_free(e.data); cllm_set_device(c->device); }
    e = tp_shard(); e.n = n; e.bytes = bytes;
    for (int i = 0; i < n; i++) { const auto * bc = (const hip_buffer_ctx *) srcs[i]->buffer->context; e.src[i] = srcs[i]->data; e.uid[i] = bc->uid; e.gen[i] = bc->gen.load(); }
    void * local = nullptr;
    cllm_set_device(c->device);
    if (cllm_malloc(&local, bytes ? bytes : 1) != CLLM_OK) return nullptr;
    for (int i = 0; i < np; i++)
        if (cllm_copy_2d(c->stream, (char *) local + pieces[i].doff, pieces[i].dpitch, pieces[i].src, pieces[i].spitch, pieces[i].width, pieces[i].rows) != CLLM_OK) { cllm_stream_sync(c->stream); cllm_free(local); return nullptr; }
    if (R.gpu == c->device) e.data = local;
    else {
        void * remote = nullptr;
        cllm_set_device(R.gpu);
        const int rc = cllm_malloc(&remote, bytes ? bytes : 1);
        cllm_set_device(c->device);
        if (rc != CLLM_OK || cllm_memcpy_peer_async(remote, R.gpu, local, c->device, bytes, c->stream) != CLLM_OK || cllm_stream_sync(c->stream) != CLLM_OK) {
            cllm_stream_sync(c->stream); cllm_free(local);
            if (remote) { cllm_set_device(R.gpu); cllm_free(remote); cllm_set_device(c->device); }
            return nullptr;
        }
        cllm_free(local);
        e.data = remote;
    }
    *built = true;
    return e.data;
}

// after a synchronize: did a bounded granule wait of the last tensor-parallel step time out?
bool tp_check_errors() {
    auto & T = g_tp;
    if (T.n <= 1 || !T.last_tp || !T.fused_ready) return true;
    T.last_tp = false;
    bool ok = true;
    for (tp_rank & R : T.r) { cllm_set_device(R.gpu); if (R.fused && cllm_tp_fused_error(R.fused)) ok = false; }
    cllm_set_device(T.r[0].gpu);
    return ok;
}
void tp_free_all() {
    auto & T = g_tp;
    for (tp_rank & R : T.r) {
        cllm_set_device(R.gpu);
        if (R.stream) cllm_stream_sync(R.stream);
        for (auto & kv : R.shards) if (kv.second.data) cllm_free(kv.second.data);
        R.shards.clear();
        for (void * p : R.kv_mem) if (p) cllm_free(p);
        R.kv_mem.clear(); R.kv_sig.clear();
        if (R.kv_table) cllm_free(R.kv_table);
        if (R.scratch) cllm_free(R.scratch);
        if (R.fused) cllm_tp_fused_destroy(R.fused);
        if (R.ev) cllm_event_destroy(R.ev);
        if (R.own_stream && R.stream) cllm_stream_destroy(R.stream);
    }
    for (void * e : T.execs) if (e) cllm_graph_destroy(e);
    T.execs.clear(); T.graph_sig.clear(); T.last_sig.clear();
    if (T.ev0) cllm_event_destroy(T.ev0);
    T.r.clear(); T.fused_ready = false; T.ev0 = nullptr; T.owner = nullptr;
}

// ---- one decode step, tensor-parallel: the state its steps share ----------------------------------------------------------------------------------------------
struct tp_lw { const ggml_tensor * wq, * wk, * wv, * bq, * bk, * bv, * wo, * wg, * wu, * wd; const float * an, * fn; float an_eps, fn_eps; };      // a layer's weights as the host holds them
struct tp_ls { void * qkv, * bias, * o, * gu, * dn; const float * an, * fn; };                                                                      // ... and one rank's shards of them
struct tp_rk { float * cs, * xa, * xb, * qkv, * att, * act; int32_t * pos; void * scores; size_t score_bytes; float * cur; };                        // where a rank keeps its inputs and intermediates
struct tp_hw { const void * wrows; const float * nw; int64_t v0, vc; };                                                                              // a rank's rows of the lm_head
struct tp_step {
    hip_backend_ctx * c; ggml_cgraph * g; const fuse_plan & P; tp_desc D;
    int N = 0, L = 0; tp_dims d;                                            // tp_check_shapes: dims, the first layer's attention, the weights and splits
    const fused_attn * A0 = nullptr;
    const ggml_tensor * emb = nullptr, * wh = nullptr; const float * curx = nullptr;      // curx: the host's residual stream behind the last layer
    ggml_type tq = GGML_TYPE_F32, to = GGML_TYPE_F32, tg = GGML_TYPE_F32, td = GGML_TYPE_F32; bool mv_head_ok = false;
    std::vector<tp_lw> W; std::vector<tp_split> S;
    std::vector<std::vector<tp_ls>> SH; bool built = false;                 // tp_make_shards (built: a shard was cut in this call, rank 0's stream must drain before the step)
    std::vector<tp_rk> X; tp_hand_over_args in; bool table = false;         // tp_ensure_scratch_and_kv
    const fused_mv * fh = nullptr; ggml_tensor * hn = nullptr, * hm = nullptr; float eps_h = 0.0f; float * logits = nullptr; bool sharded = false; std::vector<tp_hw> HW;      // tp_head_operands
    std::vector<void *> streams; std::vector<int> sgpu;                     // the distinct streams, rank order, and their GPUs
    ggml_tensor * node(int i) const { return ggml_graph_node(g, i); }
};

// a refusal before the first launch: CLLM_HIP_TP_DEBUG=1 says which one
ggml_status tp_not_taken(int line) {
    if (g_opt.tp_debug) fprintf(stderr, "[ggml-hip] tensor parallel: decode step not taken (tp_step.h:%d): un-sharded on rank 0\n", line);
    return GGML_STATUS_ABORTED;
}
#define TP_NO() tp_not_taken(__LINE__)
#define TP_TRY(expr) do { const int rc_ = (expr); if (rc_ != CLLM_OK) return rc_; } while (0)
// a launch of the step failed: say which part, leave rank 0's device current
ggml_status tp_fail(hip_backend_ctx * c, const char * what, int rc) {
    HIPB_LOG("tensor-parallel step: %s failed: %s", what, cllm_last_error());
    cllm_set_device(c->device);
    return rc == CLLM_E_ALLOC ? GGML_STATUS_ALLOC_FAILED : GGML_STATUS_FAILED;
}

// ---- the chain of residual streams and the shapes: everything is checked BEFORE the first launch ----
ggml_status tp_check_shapes(tp_step & t) {
    const fuse_plan & P = t.P; const tp_desc & D = t.D; tp_dims & d = t.d; const int N = t.N, L = t.L;
    t.emb = t.node(D.embed);
    if (!f32_vec(t.emb)) return TP_NO();
    d.H = t.emb->ne[0];
    const float * curx = (const float *) t.emb->data;
    const fused_attn & A0 = P.attns[D.layers[0].attn];
    t.A0 = &A0;
    d.hd = A0.hd; d.nh = A0.nh; d.nkv = A0.nkv; d.ML = A0.ML;
    if (d.nkv < N || d.nh % d.nkv) return TP_NO();
    d.gs = d.nh / d.nkv;
    std::vector<tp_lw> & W = t.W;
    W.resize((size_t) L);
    for (int l = 0; l < L; l++) {
        const tp_layer & Y = D.layers[l];
        const merge_group & G = P.groups[Y.gq]; const fused_attn & A = P.attns[Y.attn];
        if (G.member[0] != A.wq || G.member[1] != A.wk || G.member[2] != A.wv) return TP_NO();
        const fused_mv & fq = P.mvs[A.wq], & fk = P.mvs[A.wk], & fv = P.mvs[A.wv], & fo = P.mvs[Y.o], & fd = P.mvs[Y.down];
        const merge_group & GG = P.groups[Y.ggu];
        const fused_mv & fg = P.mvs[GG.member[0]], & fu = P.mvs[GG.member[1]];
        tp_lw & w = W[(size_t) l];
        w.wq = t.node(fq.node)->src[0]; w.wk = t.node(fk.node)->src[0]; w.wv = t.node(fv.node)->src[0]; w.wo = t.node(fo.node)->src[0];
        w.wg = t.node(fg.node)->src[0]; w.wu = t.node(fu.node)->src[0]; w.wd = t.node(fd.node)->src[0];
        w.bq = G.bias ? fq.resid_t : nullptr; w.bk = G.bias ? fk.resid_t : nullptr; w.bv = G.bias ? fv.resid_t : nullptr;
        w.an = fq.pw; w.an_eps = fq.eps; w.fn = fg.pw; w.fn_eps = fg.eps;
        if (A.hd != d.hd || A.nh != d.nh || A.nkv != d.nkv || A.ML != d.ML || A.mode != A0.mode || A.freq_base != A0.freq_base || A.n_kv != A0.n_kv) return TP_NO();
        if (fq.px != curx || fo.px != A.out || fo.resid != curx) return TP_NO();
        curx = fo.dst;
        if (fg.px != curx || fd.resid != curx) return TP_NO();
        curx = fd.dst;
        if (w.wq->ne[0] != d.H || w.wq->ne[1] != d.nh * d.hd || w.wk->ne[1] != d.nkv * d.hd || w.wv->ne[1] != d.nkv * d.hd || w.wo->ne[0] != d.nh * d.hd || w.wo->ne[1] != d.H) return TP_NO();
        if (l == 0) d.F = w.wg->ne[1];
        if (w.wg->ne[0] != d.H || w.wg->ne[1] != d.F || w.wu->ne[1] != d.F || w.wd->ne[0] != d.F || w.wd->ne[1] != d.H || w.wg->type != w.wu->type) return TP_NO();
        if (w.wq->type != W[0].wq->type || w.wo->type != W[0].wo->type || w.wg->type != W[0].wg->type || w.wd->type != W[0].wd->type) return TP_NO();
    }
    const ggml_tensor * wh = nullptr;
    if (D.head >= 0) {
        const fused_mv & fh = P.mvs[D.head];
        if (fh.px != curx) return TP_NO();
        wh = t.node(fh.node)->src[0];
    } else {
        const ggml_tensor * hn = t.node(D.head_norm);
        if (!hn->src[0]->src[0] || hn->src[0]->src[0]->data != (const void *) curx || ggml_nelements(hn) != d.H) return TP_NO();
        wh = t.node(D.head_mm)->src[0];
    }
    t.curx = curx; t.wh = wh;
    auto kind = [](ggml_type ty) { return (int64_t)(ty == GGML_TYPE_Q4_K ? 256 : 32); };
    const ggml_type tq = t.tq = W[0].wq->type, to = t.to = W[0].wo->type, tg = t.tg = W[0].wg->type, td = t.td = W[0].wd->type;
    t.mv_head_ok = is_q(wh->type) && wh->ne[2] == 1 && wh->ne[3] == 1 && wh->nb[1] == ggml_row_size(wh->type, wh->ne[0]) && !((uintptr_t) wh->data & 15) && !(wh->nb[1] & 15) && wh->ne[0] == d.H;
    // what the two tensor-parallel forms take (gemv_tp.hip) -- and the whole-KV-group / whole-quant-block splits
    if (d.H % kind(tq) || d.H % kind(tg) || d.H % kind(wh->type) || d.H > 16384 || d.H % 4) return TP_NO();
    const int64_t fblk = ggml_blck_size(td), nfb = d.F / fblk;
    if (d.F % fblk || nfb < N || d.F % 8) return TP_NO();
    t.S.resize((size_t) N);
    for (int k = 0; k < N; k++) {
        tp_split & s = t.S[(size_t) k];
        int64_t b0, bc;
        cllm_tp_split(d.nkv, N, k, &s.kv0, &s.kvc); cllm_tp_split(nfb, N, k, &b0, &bc);
        s.f0 = b0 * fblk; s.fc = bc * fblk;
        const int64_t qc = s.kvc * d.gs * d.hd, q0 = s.kv0 * d.gs * d.hd;
        if (s.kvc < 1 || qc % kind(to) || q0 % ggml_blck_size(to) || qc > 32768 || s.fc % kind(td) || s.fc > 32768 || (s.fc % 8) ||
            !cllm_attn_decode_supported((int)(s.kvc * d.gs), (int) s.kvc, (int) d.hd, d.ML)) return TP_NO();
    }
    return GGML_STATUS_SUCCESS;
}

// ---- shards (first step, or after the host rewrote a weight) ----
ggml_status tp_fail_shard(hip_backend_ctx * c) {
    HIPB_LOG("tensor parallel: a weight shard could not be made (%s) -- running un-sharded on rank 0 from now on", cllm_last_error());
    g_tp.broken = true; cllm_set_device(c->device);
    return TP_NO();
}
const float * tp_replicate(tp_step & t, int k, const float * p, size_t bytes, const ggml_tensor * owner) {      // a small F32 tensor every rank reads (norm weights)
    if (g_tp.r[(size_t) k].gpu == t.c->device) return p;
    const ggml_tensor * src[1] = { owner };
    tp_piece pc = { p, bytes, bytes, 1, 0, bytes };
    return (const float *) tp_get_shard(t.c, k, src, 1, &pc, 1, bytes, &t.built);
}
const ggml_tensor * tp_norm_owner(const tp_step & t, const fused_mv & f) { return t.node(f.node)->src[1]->src[1]; }      // MUL_MAT(w, MUL(RMS_NORM(x), weight)): the weight tensor
ggml_status tp_make_shards(tp_step & t) {
    hip_backend_ctx * c = t.c; const fuse_plan & P = t.P; const tp_desc & D = t.D; const tp_dims & d = t.d; const int N = t.N, L = t.L;
    const ggml_type to = t.to, td = t.td;
    bool & built = t.built;
    t.SH.assign((size_t) N, std::vector<tp_ls>((size_t) L));
    for (int k = 0; k < N; k++) {
        const tp_split & s = t.S[(size_t) k];
        const int64_t qr0 = s.kv0 * d.gs * d.hd, qrc = s.kvc * d.gs * d.hd, kr0 = s.kv0 * d.hd, krc = s.kvc * d.hd;
        for (int l = 0; l < L; l++) {
            const tp_lw & w = t.W[(size_t) l]; tp_ls & o = t.SH[(size_t) k][(size_t) l];
            const tp_layer & Y = D.layers[l];
            {   // q | k | v rows of this rank's KV groups
                const size_t rb = w.wq->nb[1];
                const ggml_tensor * src[3] = { w.wq, w.wk, w.wv };
                tp_piece pc[3] = { { (const char *) w.wq->data + qr0 * rb, qrc * rb, qrc * rb, 1, 0, qrc * rb }, { (const char *) w.wk->data + kr0 * rb, krc * rb, krc * rb, 1, (size_t) qrc * rb, krc * rb },
                                   { (const char *) w.wv->data + kr0 * rb, krc * rb, krc * rb, 1, (size_t)(qrc + krc) * rb, krc * rb } };
                if (w.wk->nb[1] != rb || w.wv->nb[1] != rb || !(o.qkv = tp_get_shard(c, k, src, 3, pc, 3, (size_t)(qrc + 2 * krc) * rb, &built))) return tp_fail_shard(c);
                o.bias = nullptr;
                if (w.bq) {
                    const ggml_tensor * bs[3] = { w.bq, w.bk, w.bv };
                    tp_piece bp[3] = { { (const char *) w.bq->data + qr0 * 4, (size_t) qrc * 4, (size_t) qrc * 4, 1, 0, (size_t) qrc * 4 }, { (const char *) w.bk->data + kr0 * 4, (size_t) krc * 4, (size_t) krc * 4, 1, (size_t) qrc * 4, (size_t) krc * 4 },
                                       { (const char *) w.bv->data + kr0 * 4, (size_t) krc * 4, (size_t) krc * 4, 1, (size_t)(qrc + krc) * 4, (size_t) krc * 4 } };
                    if (!(o.bias = tp_get_shard(c, k, bs, 3, bp, 3, (size_t)(qrc + 2 * krc) * 4, &built))) return tp_fail_shard(c);
                }
            }
            {   // o: the quant blocks of K that belong to this rank's heads
                const size_t wb = ggml_row_size(to, qrc), ob = ggml_row_size(to, qr0);
                const ggml_tensor * src[1] = { w.wo };
                tp_piece pc = { (const char *) w.wo->data + ob, w.wo->nb[1], wb, (size_t) d.H, 0, wb };
                if (!(o.o = tp_get_shard(c, k, src, 1, &pc, 1, wb * (size_t) d.H, &built))) return tp_fail_shard(c);
            }
            {   // gate / up rows [f0, f0 + fc), alternating
                const size_t rb = w.wg->nb[1];
                const ggml_tensor * src[2] = { w.wg, w.wu };
                tp_piece pc[2] = { { (const char *) w.wg->data + s.f0 * rb, rb, rb, (size_t) s.fc, 0, 2 * rb }, { (const char *) w.wu->data + s.f0 * rb, rb, rb, (size_t) s.fc, rb, 2 * rb } };
                if (w.wu->nb[1] != rb || !(o.gu = tp_get_shard(c, k, src, 2, pc, 2, 2 * (size_t) s.fc * rb, &built))) return tp_fail_shard(c);
            }
            {   // down: the quant blocks [f0 / blk, (f0 + fc) / blk) of every row
                const size_t wb = ggml_row_size(td, s.fc), ob = ggml_row_size(td, s.f0);
                const ggml_tensor * src[1] = { w.wd };
                tp_piece pc = { (const char *) w.wd->data + ob, w.wd->nb[1], wb, (size_t) d.H, 0, wb };
                if (!(o.dn = tp_get_shard(c, k, src, 1, &pc, 1, wb * (size_t) d.H, &built))) return tp_fail_shard(c);
            }
            o.an = tp_replicate(t, k, w.an, (size_t) d.H * 4, tp_norm_owner(t, P.mvs[P.attns[Y.attn].wq]));
            o.fn = tp_replicate(t, k, w.fn, (size_t) d.H * 4, tp_norm_owner(t, P.mvs[P.groups[Y.ggu].member[0]]));
            if (!o.an || !o.fn) return tp_fail_shard(c);
        }
    }
    return GGML_STATUS_SUCCESS;
}

// ---- per-rank scratch: [cos/sin 1 KB][pos 256 B][x ping][x pong][q|k|v][attention out][SiLU*up][scores of the long-context attention] ----
struct tp_layout { size_t cs, pos, xa, xb, qkv, att, act, scores, score_bytes, total; };      // byte offsets into tp_rank::scratch
tp_layout tp_rank_layout(const tp_dims & d, const tp_split & s, int64_t n_kv) {
    tp_layout o; size_t b = 0;
    o.cs = b; b += 1024; o.pos = b; b += 256;
    o.xa = b; b += al256((size_t) d.H * 4); o.xb = b; b += al256((size_t) d.H * 4);
    o.qkv = b; b += al256((size_t)(s.kvc * (d.gs + 2) * d.hd) * 4); o.att = b; b += al256((size_t)(s.kvc * d.gs * d.hd) * 4);
    o.act = b; b += al256((size_t) s.fc * 4);
    o.score_bytes = cllm_attn_decode_wsize(n_kv, (int)(s.kvc * d.gs), d.ML); o.scores = b; b += al256(o.score_bytes);
    o.total = b;
    return o;
}
// every rank's scratch (grown if need be; pointer arithmetic only: nothing is launched before the signature is known), the hand-over's arguments, and the
// KV shards: table of { host K, host V, shard K, shard V } per layer on every rank's GPU
ggml_status tp_ensure_scratch_and_kv(tp_step & t) {
    auto & T = g_tp; hip_backend_ctx * c = t.c; const fuse_plan & P = t.P; const tp_desc & D = t.D; const tp_dims & d = t.d; const int N = t.N, L = t.L; const fused_attn & A0 = *t.A0;
    t.table = d.hd == 64 || d.hd == 128;
    t.X.resize((size_t) N);
    t.in.ea = desc(t.emb->src[0]); t.in.eb = desc(t.emb->src[1]); t.in.ed = desc(t.emb); t.in.pos_src = A0.pos; t.in.hbytes = (size_t) d.H * 4;
    for (int k = 0; k < N; k++) {
        tp_rank & R = T.r[(size_t) k]; tp_rk & x = t.X[(size_t) k];
        const tp_layout o = tp_rank_layout(d, t.S[(size_t) k], A0.n_kv);
        const size_t need = o.total;
        if (need > R.scratch_bytes) {
            cllm_set_device(R.gpu); cllm_stream_sync(R.stream);
            if (R.scratch) cllm_free(R.scratch);
            R.scratch = nullptr; R.scratch_bytes = 0;
            void * p = nullptr;
            if (cllm_malloc(&p, need + need / 4) != CLLM_OK) { cllm_set_device(c->device); return GGML_STATUS_ALLOC_FAILED; }
            R.scratch = (char *) p; R.scratch_bytes = need + need / 4;
        }
        char * b = R.scratch;
        x.cs = (float *)(b + o.cs); x.pos = (int32_t *)(b + o.pos); x.xa = (float *)(b + o.xa); x.xb = (float *)(b + o.xb);
        x.qkv = (float *)(b + o.qkv); x.att = (float *)(b + o.att); x.act = (float *)(b + o.act);
        x.score_bytes = o.score_bytes; x.scores = o.score_bytes ? (void *)(b + o.scores) : nullptr;
        x.cur = x.xa;
        t.in.xa.push_back(x.xa); t.in.pos.push_back(x.pos);
    }
    const uint64_t epoch = g_tp_kv_epoch.load();
    for (int k = 0; k < N; k++) {
        tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k];
        std::vector<const void *> sig; sig.reserve((size_t) 2 * L);
        for (int l = 0; l < L; l++) { const fused_attn & A = P.attns[D.layers[l].attn]; sig.push_back(A.k_cache); sig.push_back(A.v_cache); }
        const size_t kd = (size_t)(s.kvc * d.hd);
        if (sig != R.kv_sig || R.kv_dims[0] != kd || R.kv_dims[1] != (size_t) d.ML || R.kv_dims[2] != (size_t) s.kv0) {
            cllm_set_device(R.gpu); cllm_stream_sync(R.stream);
            for (void * p : R.kv_mem) if (p) cllm_free(p);
            R.kv_mem.assign((size_t) 2 * L, nullptr);
            if (!R.kv_table && cllm_malloc(&R.kv_table, 4096 * 32) != CLLM_OK) { cllm_set_device(c->device); return GGML_STATUS_ALLOC_FAILED; }
            if (L > 4096) { cllm_set_device(c->device); return TP_NO(); }
            std::vector<void *> tab((size_t) 4 * L);
            for (int l = 0; l < L; l++) {
                for (int h = 0; h < 2; h++) if (cllm_malloc(&R.kv_mem[(size_t)(2 * l + h)], kd * (size_t) d.ML * 2) != CLLM_OK) { cllm_set_device(c->device); return GGML_STATUS_ALLOC_FAILED; }
                tab[(size_t) 4 * l] = (void *) sig[(size_t) 2 * l]; tab[(size_t) 4 * l + 1] = (void *) sig[(size_t) 2 * l + 1]; tab[(size_t) 4 * l + 2] = R.kv_mem[(size_t) 2 * l]; tab[(size_t) 4 * l + 3] = R.kv_mem[(size_t) 2 * l + 1];
            }
            if (cllm_memcpy_h2d(R.kv_table, tab.data(), tab.size() * sizeof(void *), nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) { cllm_set_device(c->device); return GGML_STATUS_FAILED; }
            R.kv_sig = sig; R.kv_dims[0] = kd; R.kv_dims[1] = (size_t) d.ML; R.kv_dims[2] = (size_t) s.kv0; R.kv_valid = 0;
        }
        if (R.kv_epoch != epoch) { R.kv_valid = 0; R.kv_epoch = epoch; }
    }
    cllm_set_device(c->device);
    if (t.built && cllm_stream_sync(c->stream) != CLLM_OK) return GGML_STATUS_FAILED;
    return GGML_STATUS_SUCCESS;
}

// ---- the head's operands.  Sharded by ROWS of the lm_head (default; CLLM_HIP_TP_HEAD=0: all of it on rank 0): every rank folds the last all-reduce into its own residual
//      stream and writes its logit rows straight into the host's logits tensor in rank 0's memory (a peer store from another GPU); a row's arithmetic does not change, so the
//      logits are the bits rank 0 alone would have produced from the same residual stream.  chatllm keeps the normalised hidden state as a graph OUTPUT: rank 0 also runs that node.
ggml_status tp_head_operands(tp_step & t) {
    auto & T = g_tp; hip_backend_ctx * c = t.c; const fuse_plan & P = t.P; const tp_desc & D = t.D; const tp_dims & d = t.d; const int N = t.N; const ggml_tensor * wh = t.wh;
    const fused_mv * fh = t.fh = D.head >= 0 ? &P.mvs[D.head] : nullptr;
    ggml_tensor * hn = t.hn = D.head >= 0 ? nullptr : t.node(D.head_norm), * hm = t.hm = D.head >= 0 ? nullptr : t.node(D.head_mm);
    const float * norm_w = fh ? fh->pw : (const float *) hn->src[1]->data;
    const ggml_tensor * norm_t = fh ? tp_norm_owner(t, *fh) : hn->src[1];
    t.eps_h = fh ? fh->eps : 0.0f;
    if (!fh) memcpy(&t.eps_h, hn->src[0]->op_params, 4);
    t.logits = fh ? fh->dst : (float *) hm->data;
    const int64_t V = wh->ne[1];
    const bool sharded = t.sharded = g_opt.tp_head && V >= 8 * (int64_t) N && t.mv_head_ok;
    t.HW.resize((size_t) N);
    for (int k = 0; k < (sharded ? N : 1); k++) {
        tp_rank & R = T.r[(size_t) k]; tp_hw & h = t.HW[(size_t) k];
        h.v0 = 0; h.vc = V;
        if (sharded) cllm_tp_split(V, N, k, &h.v0, &h.vc);
        // this rank's rows of the lm_head: the host's tensor itself where the rank shares rank 0's GPU, else a copy made on first use
        h.wrows = (const char *) wh->data + (size_t) h.v0 * wh->nb[1]; h.nw = norm_w;
        if (R.gpu != c->device) {
            const ggml_tensor * src[1] = { wh };
            tp_piece pc = { h.wrows, (size_t) h.vc * wh->nb[1], (size_t) h.vc * wh->nb[1], 1, 0, (size_t) h.vc * wh->nb[1] };
            bool b2 = false;
            h.wrows = tp_get_shard(c, k, src, 1, &pc, 1, (size_t) h.vc * wh->nb[1], &b2);
            h.nw = tp_replicate(t, k, norm_w, (size_t) d.H * 4, norm_t);
            if (!h.wrows || !h.nw) { HIPB_LOG("tensor parallel: the lm_head shard of rank %d could not be made (%s)", k, cllm_last_error()); cllm_set_device(c->device); return GGML_STATUS_FAILED; }
        }
    }
    if (!fh && !sharded) {
        cllm_tensor da = desc(hm->src[0]), db = desc(hm->src[1]);
        cllm_set_device(c->device);
        if (int rc = ensure_wdata(c, cllm_mul_mat_wsize(&da, &db))) return tp_fail(c, "the lm_head's scratch", rc);
    }
    return GGML_STATUS_SUCCESS;
}

// ---- launch-list replay per stream (as be_graph_compute does for one stream): everything a launch depends on goes into a signature ----
std::vector<uint64_t> tp_sign(const tp_step & t) {
    const auto & T = g_tp; const tp_dims & d = t.d; const int N = t.N, L = t.L; const ggml_tensor * hn = t.hn, * hm = t.hm;
    std::vector<uint64_t> sig;
    auto put = [&](const void * p) { sig.push_back((uint64_t)(uintptr_t) p); };
    auto putf = [&](float f) { uint32_t u; memcpy(&u, &f, 4); sig.push_back(u); };
    sig.push_back((uint64_t) N); sig.push_back((uint64_t) L); sig.push_back((uint64_t) d.H); sig.push_back((uint64_t) d.F); sig.push_back((uint64_t) d.hd); sig.push_back((uint64_t) d.ML);
    sig.push_back((uint64_t) t.tq | (uint64_t) t.to << 8 | (uint64_t) t.tg << 16 | (uint64_t) t.td << 24 | (uint64_t) t.wh->type << 32); sig.push_back((uint64_t) t.A0->mode); putf(t.A0->freq_base); putf(t.eps_h);
    sig.push_back((uint64_t) t.sharded | (uint64_t)(t.fh != nullptr) << 1 | (uint64_t) t.table << 2);
    put(t.logits); put(t.curx); put(hn ? hn->data : nullptr); put(hn ? hn->src[0]->src[0]->data : nullptr); put(hm ? hm->src[0]->data : nullptr); put(hm ? hm->src[1]->data : nullptr); put(t.c->wdata);
    for (int k = 0; k < N; k++) {
        const tp_rank & R = T.r[(size_t) k]; const tp_split & s0 = t.S[(size_t) k]; const tp_rk & x = t.X[(size_t) k];
        put(R.stream); put(R.fused); put(R.scratch); put(R.kv_table); sig.push_back((uint64_t) s0.kv0 << 32 | (uint64_t) s0.kvc); sig.push_back((uint64_t) s0.f0 << 32 | (uint64_t) s0.fc);
        sig.push_back((uint64_t)(x.score_bytes != 0));
        put(t.HW[(size_t) k].wrows); put(t.HW[(size_t) k].nw); sig.push_back((uint64_t) t.HW[(size_t) k].v0); sig.push_back((uint64_t) t.HW[(size_t) k].vc);
        for (int l = 0; l < L; l++) { const tp_ls & o = t.SH[(size_t) k][(size_t) l]; put(o.qkv); put(o.bias); put(o.o); put(o.gu); put(o.dn); put(o.an); put(o.fn); put(R.kv_mem[(size_t) 2 * l]); put(R.kv_mem[(size_t) 2 * l + 1]); putf(t.W[(size_t) l].an_eps); putf(t.W[(size_t) l].fn_eps); }
    }
    return sig;
}

// ---- what stands in front of the sharded launches: the embedding row on rank 0, that row and the position handed to every rank (queued on rank 0's stream: behind the GET_ROWS
//      and behind everything an earlier un-sharded graph wrote), the ranks' streams made to wait for them ----
int tp_hand_over(hip_backend_ctx * c, const tp_hand_over_args & a) {
    auto & T = g_tp; void * st0 = c->stream;
    cllm_set_device(c->device);
    cllm_tensor ed = a.ed;
    TP_TRY(cllm_op_get_rows(st0, &a.ea, &a.eb, &ed));
    bool remote = false;
    for (int k = 0; k < T.n; k++) {
        tp_rank & R = T.r[(size_t) k];
        TP_TRY(cllm_memcpy_peer_async(a.xa[(size_t) k], R.gpu, a.ed.data, c->device, a.hbytes, st0));
        TP_TRY(cllm_memcpy_peer_async(a.pos[(size_t) k], R.gpu, a.pos_src, c->device, 4, st0));
        remote = remote || R.own_stream;
    }
    if (remote) {
        TP_TRY(cllm_event_record(T.ev0, st0));
        for (int k = 0; k < T.n; k++) if (T.r[(size_t) k].own_stream) { cllm_set_device(T.r[(size_t) k].gpu); TP_TRY(cllm_stream_wait_event(T.r[(size_t) k].stream, T.ev0)); }
    }
    return CLLM_OK;
}
// ... and behind them: everything joins rank 0's stream
int tp_join(hip_backend_ctx * c) {
    for (tp_rank & R : g_tp.r)
        if (R.own_stream) { cllm_set_device(R.gpu); TP_TRY(cllm_event_record(R.ev, R.stream)); cllm_set_device(c->device); TP_TRY(cllm_stream_wait_event(c->stream, R.ev)); }
    return CLLM_OK;
}
// the cache shards brought up to date: rows the host's cache has and the shard has not (a prompt ran un-sharded, a session was loaded ...)
int tp_refresh_kv(tp_step & t) {
    const tp_dims & d = t.d; const fused_attn & A0 = *t.A0;
    for (int k = 0; k < t.N; k++) {
        tp_rank & R = g_tp.r[(size_t) k]; const tp_split & s = t.S[(size_t) k];
        cllm_set_device(R.gpu);
        if (R.kv_valid < A0.n_kv - 1) TP_TRY(cllm_op_kv_shard_copy(R.stream, R.kv_table, t.L, (int)(s.kvc * d.hd), (int)(d.nkv * d.hd), (int)(s.kv0 * d.hd), d.ML, R.kv_valid, A0.n_kv - 1, nullptr, 0));
        R.kv_valid = A0.n_kv;
    }
    return CLLM_OK;
}
int tp_pre_step(tp_step & t) { TP_TRY(tp_hand_over(t.c, t.in)); return tp_refresh_kv(t); }
int tp_launch_graphs(const std::vector<void *> & streams, const std::vector<int> & gpus) {
    for (size_t q = 0; q < streams.size(); q++) { cllm_set_device(gpus[q]); TP_TRY(cllm_graph_launch(g_tp.execs[q], streams[q])); }
    return CLLM_OK;
}

cllm_tensor tp_wdesc(ggml_type ty, int64_t K, int64_t rows, void * data) {
    cllm_tensor w; w.type = (int32_t) ty; w.ne[0] = K; w.ne[1] = rows; w.ne[2] = w.ne[3] = 1;
    w.nb[0] = ggml_type_size(ty); w.nb[1] = ggml_row_size(ty, K); w.nb[2] = w.nb[3] = w.nb[1] * (size_t) rows; w.data = data; return w;
}
// ---- the launches of the step proper.  only == nullptr: every rank, site by site (ranks that share a stream must be issued in this order: a gather never polls for a launch
//      behind it); only == a stream: the ranks of that stream alone, same order -- what is captured into that stream's graph ----
int tp_issue(tp_step & t, void * only) {
    auto & T = g_tp; hip_backend_ctx * c = t.c; const fuse_plan & P = t.P; const tp_desc & D = t.D; const tp_dims & d = t.d; const int N = t.N, L = t.L; const fused_attn & A0 = *t.A0;
    const bool table = t.table, sharded = t.sharded; const fused_mv * fh = t.fh; ggml_tensor * hn = t.hn, * hm = t.hm;
    auto mine = [&](int k) { return !only || T.r[(size_t) k].stream == only; };
    for (int k = 0; k < N; k++) if (mine(k)) {
        tp_rank & R = T.r[(size_t) k]; tp_rk & x = t.X[(size_t) k];
        cllm_set_device(R.gpu);
        x.cur = x.xa;
        TP_TRY(cllm_tp_fused_advance(R.fused, R.stream));
        if (table) TP_TRY(cllm_op_rope_table(R.stream, x.pos, (int) d.hd, A0.freq_base, x.cs));
    }
    int pend = -1;                                // the site whose partial sums are not yet in the residual stream
    for (int l = 0; l < L; l++) {
        const fused_attn & A = P.attns[D.layers[l].attn];
        for (int k = 0; k < N; k++) if (mine(k)) {    // q | k | v (+ the all-reduce of the previous down projection + residual + RMS_NORM)
            tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k]; const tp_ls & o = t.SH[(size_t) k][(size_t) l];
            cllm_set_device(R.gpu);
            cllm_tensor w = tp_wdesc(t.tq, d.H, s.kvc * (d.gs + 2) * d.hd, o.qkv);
            if (pend < 0) TP_TRY(cllm_op_mul_mat_vec_fused(R.stream, &w, 1, x.cur, o.an, t.W[(size_t) l].an_eps, 0, (const float *) o.bias, x.qkv));
            else { float * nx = x.cur == x.xa ? x.xb : x.xa; TP_TRY(cllm_op_mul_mat_vec_tp_gather(R.stream, &w, x.cur, o.an, t.W[(size_t) l].an_eps, 0, (const float *) o.bias, x.qkv, R.fused, pend, nx)); x.cur = nx; }
        }
        for (int k = 0; k < N; k++) if (mine(k)) {    // RoPE + cache rows + attention over this rank's heads
            tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k];
            cllm_set_device(R.gpu);
            TP_TRY(cllm_op_rope_kv_attn_decode(R.stream, x.qkv, x.pos, table ? x.cs : nullptr, A.freq_base, A.n_kv, (int)(s.kvc * d.gs), (int) s.kvc, (int) d.hd, A.mode, R.kv_mem[(size_t) 2 * l], R.kv_mem[(size_t) 2 * l + 1], d.ML,
                                               x.att, x.scores, x.score_bytes));
        }
        for (int k = 0; k < N; k++) if (mine(k)) {    // o: partial rows -> every rank
            tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k]; const tp_ls & o = t.SH[(size_t) k][(size_t) l];
            cllm_set_device(R.gpu);
            cllm_tensor w = tp_wdesc(t.to, s.kvc * d.gs * d.hd, d.H, o.o);
            TP_TRY(cllm_op_mul_mat_vec_tp_scatter(R.stream, &w, 2, x.att, R.fused, 2 * l));
        }
        for (int k = 0; k < N; k++) if (mine(k)) {    // gate / up with SiLU * up (+ the all-reduce of o + residual + RMS_NORM)
            tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k]; const tp_ls & o = t.SH[(size_t) k][(size_t) l];
            cllm_set_device(R.gpu);
            cllm_tensor w = tp_wdesc(t.tg, d.H, 2 * s.fc, o.gu);
            float * nx = x.cur == x.xa ? x.xb : x.xa;
            TP_TRY(cllm_op_mul_mat_vec_tp_gather(R.stream, &w, x.cur, o.fn, t.W[(size_t) l].fn_eps, 1, nullptr, x.act, R.fused, 2 * l, nx));
            x.cur = nx;
        }
        for (int k = 0; k < N; k++) if (mine(k)) {    // down: partial rows -> every rank
            tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k]; const tp_ls & o = t.SH[(size_t) k][(size_t) l];
            cllm_set_device(R.gpu);
            cllm_tensor w = tp_wdesc(t.td, s.fc, d.H, o.dn);
            TP_TRY(cllm_op_mul_mat_vec_tp_scatter(R.stream, &w, 2, x.act, R.fused, 2 * l + 1));
        }
        pend = 2 * l + 1;
    }
    for (int k = 0; k < (sharded ? N : 1); k++) if (mine(k)) {      // the head
        tp_rank & R = T.r[(size_t) k]; tp_rk & x = t.X[(size_t) k]; const tp_hw & h = t.HW[(size_t) k];
        cllm_set_device(R.gpu);
        cllm_tensor w = tp_wdesc(t.wh->type, d.H, h.vc, (void *) h.wrows);
        float * nx = x.cur == x.xa ? x.xb : x.xa;
        if (fh) {                             // a fused norm + lm_head: its RMS_NORM prologue takes the last all-reduce
            TP_TRY(cllm_op_mul_mat_vec_tp_gather(R.stream, &w, x.cur, h.nw, t.eps_h, 0, nullptr, t.logits + h.v0, R.fused, pend, nx));
        } else {                              // chatllm's head: the last all-reduce lands in the residual stream (rank 0: the host's tensor), then norm + rows
            // (sharded: into the rank's own scratch -- ggml-alloc may have placed the logits on the freed block of the host's residual tensor, and the other ranks' rows land
            //  there while this rank's launch still reads its input; un-sharded: the host's residual tensor, as on one device)
            float * xfin = (k == 0 && !sharded) ? (float *) t.curx : nx;
            TP_TRY(cllm_op_tp_gather_residual(R.stream, x.cur, d.H, R.fused, pend, xfin));
            if (k == 0) {
                cllm_tensor dx = desc(hn->src[0]->src[0]), dwt = as_vec(desc(hn->src[1]), hn->ne[0]), dn = desc(hn);
                dx.data = xfin;
                TP_TRY(cllm_op_rms_norm_mul(R.stream, &dx, &dwt, &dn, t.eps_h));
            }
            if (sharded) TP_TRY(cllm_op_mul_mat_vec_fused(R.stream, &w, 1, xfin, h.nw, t.eps_h, 0, nullptr, t.logits + h.v0));      // (norm + quantize in the prologue: the bits of the two nodes)
            else {
                cllm_tensor da = desc(hm->src[0]), db = desc(hm->src[1]), dd = desc(hm);
                TP_TRY(cllm_op_mul_mat(R.stream, &da, &db, &dd, c->wdata, c->wsize));
            }
        }
    }
    for (int k = 0; k < N; k++) if (mine(k)) {    // this step's cache row back into the host's caches
        tp_rank & R = T.r[(size_t) k]; const tp_split & s = t.S[(size_t) k]; tp_rk & x = t.X[(size_t) k];
        cllm_set_device(R.gpu);
        TP_TRY(cllm_op_kv_shard_copy(R.stream, R.kv_table, L, (int)(s.kvc * d.hd), (int)(d.nkv * d.hd), (int)(s.kv0 * d.hd), d.ML, 0, 0, x.pos, 1));
    }
    return CLLM_OK;
}

// ---- the replay ladder of the sharded step: a step running ahead is resolved; else a list equal to the captured one is replayed; else the second identical list in a row is
//      captured, one graph per distinct stream (ranks on distinct GPUs: one each; virtual ranks: one for all), and launched; else every launch is issued (CLLM_HIP_TP_GRAPH=0:
//      always).  Every path but the hit runs the pre-step first ----
ggml_status tp_replay_or_issue(tp_step & t, const std::vector<uint64_t> & sig, const std::vector<hip_backend_ctx::scalar_set> & cur_sets, bool & replayed, bool & ahead_hit) {
    auto & T = g_tp; hip_backend_ctx * c = t.c;
    const bool tp_graph = g_opt.tp_graph && !T.graph_broken;
    replayed = ahead_hit = false;
    if (c->ahead.inflight) {                       // a sharded step is running ahead of the host (tp_ahead_replay): is it this one?
        const int hr = ahead_resolve(c, c->ahead.tp && T.rp.valid && !T.execs.empty() && sig == T.graph_sig && T.rp.n_kv == t.A0->n_kv, cur_sets);
        if (hr < 0) return GGML_STATUS_FAILED;
        ahead_hit = hr == 1;
    }
    if (ahead_hit) { replayed = true; T.replays++; return GGML_STATUS_SUCCESS; }
    if (int rc = tp_pre_step(t)) return tp_fail(c, "the hand-over to the ranks", rc);
    if (tp_graph && T.execs.size() == t.streams.size() && !T.execs.empty() && sig == T.graph_sig) {
        if (int rc = tp_launch_graphs(t.streams, t.sgpu)) return tp_fail(c, "the captured graphs' launch", rc);
        replayed = true; T.replays++;
    } else if (tp_graph && sig == T.last_sig) {      // second time in a row: capture one graph per stream, then launch them
        if (!T.execs.empty()) { for (size_t q = 0; q < t.streams.size(); q++) { cllm_set_device(t.sgpu[q]); cllm_stream_sync(t.streams[q]); } }      // (a replaced graph may still be running)
        for (void * e : T.execs) if (e) cllm_graph_destroy(e);
        T.execs.clear(); T.graph_sig.clear();
        bool ok = true;
        for (size_t q = 0; q < t.streams.size() && ok; q++) {
            cllm_set_device(t.sgpu[q]);
            if (cllm_graph_capture_begin(t.streams[q]) != CLLM_OK) { ok = false; break; }
            const int rs = tp_issue(t, t.streams[q]);
            void * exec = nullptr;
            cllm_set_device(t.sgpu[q]);
            const int rc = cllm_graph_capture_end(t.streams[q], &exec);
            if (rs != CLLM_OK || rc != CLLM_OK || !exec) { if (exec) cllm_graph_destroy(exec); ok = false; break; }
            T.execs.push_back(exec);
        }
        if (!ok) {                                 // nothing ran (captures execute nothing): issue the step the plain way, and stop trying
            HIPB_LOG("tensor parallel: launch-list capture failed (%s): issuing the launches of every step from now on", cllm_last_error());
            for (void * e : T.execs) if (e) cllm_graph_destroy(e);
            T.execs.clear(); T.graph_broken = true;
            if (int rc = tp_issue(t, nullptr)) return tp_fail(c, "a sharded launch", rc);
        } else {
            T.graph_sig = sig; T.captures++;
            if (int rc = tp_launch_graphs(t.streams, t.sgpu)) return tp_fail(c, "the captured graphs' launch", rc);
            replayed = true;
        }
    } else if (int rc = tp_issue(t, nullptr)) return tp_fail(c, "a sharded launch", rc);
    return GGML_STATUS_SUCCESS;
}

// one decode step, tensor-parallel.  GGML_STATUS_ABORTED = "not taken, nothing launched" (the caller runs the graph un-sharded on rank 0)
ggml_status tp_graph_compute(hip_backend_ctx * c, ggml_cgraph * g, fuse_plan & P, const std::vector<hip_backend_ctx::scalar_set> & cur_sets, bool * replayed_out) {
    auto & T = g_tp;
    if (T.broken) return GGML_STATUS_ABORTED;
    tp_step t{ c, g, P };
    if (!tp_extract(g, P, t.D)) {
        if (g_opt.tp_debug) HIPB_LOG("tensor parallel: a %d-node graph is not the decode step (%zu layers matched, embed %d, head %d/%d/%d): un-sharded on rank 0", ggml_graph_n_nodes(g), t.D.layers.size(), t.D.embed, t.D.head, t.D.head_norm, t.D.head_mm);
        return GGML_STATUS_ABORTED;
    }
    const int N = t.N = T.n, L = t.L = (int) t.D.layers.size();
    ggml_status s = tp_check_shapes(t);
    if (s != GGML_STATUS_SUCCESS) return s;
    if (tp_ensure_group(c, 2 * L, (size_t) t.d.H) != CLLM_OK) { HIPB_LOG("tensor parallel: %s -- running un-sharded on rank 0 from now on", cllm_last_error()); T.broken = true; cllm_set_device(c->device); return TP_NO(); }
    if (!T.told) { T.told = true; HIPB_LOG("tensor parallel: %d ranks behind one ggml device (%d layers; KV heads / FFN features of rank 0: %lld / %lld of %d / %lld)", N, L, (long long) t.S[0].kvc, (long long) t.S[0].fc, t.d.nkv, (long long) t.d.F); }
    if ((s = tp_make_shards(t)) != GGML_STATUS_SUCCESS) return s;
    if ((s = tp_ensure_scratch_and_kv(t)) != GGML_STATUS_SUCCESS) return s;
    if ((s = tp_head_operands(t)) != GGML_STATUS_SUCCESS) return s;
    std::vector<uint64_t> sig = tp_sign(t);
    for (const tp_rank & R : T.r) {               // the distinct streams, rank order
        bool seen = false;
        for (void * q : t.streams) seen = seen || q == R.stream;
        if (!seen) { t.streams.push_back(R.stream); t.sgpu.push_back(R.gpu); }
    }
    bool replayed = false, ahead_hit = false;
    if ((s = tp_replay_or_issue(t, sig, cur_sets, replayed, ahead_hit)) != GGML_STATUS_SUCCESS) return s;
    T.last_sig.swap(sig);
    if (!ahead_hit) if (int rc = tp_join(c)) return tp_fail(c, "the join into rank 0's stream", rc);
    // what a step started ahead of the host will need (tp_ahead_replay): valid while the captured graphs are
    T.rp.valid = replayed && !T.execs.empty();
    if (T.rp.valid) { T.rp.in = t.in; T.rp.n_kv = t.A0->n_kv; T.rp.streams = t.streams; T.rp.sgpu = t.sgpu; }
    *replayed_out = replayed;
    cllm_set_device(c->device);
    T.steps++; T.last_tp = true;
    if (g_opt.stats) HIPB_LOG("HIP0 graph_compute: %d nodes -> tensor parallel over %d ranks: %d launches per rank (%d layers x 5 + head%s)%s, all-reduce fused into the mat-vecs", ggml_graph_n_nodes(g), N, 5 * L + 6, L,
                          t.sharded ? ", lm_head rows sharded" : "", ahead_hit ? ", started ahead of the host" : replayed ? ", replayed from the captured graphs" : "");
    return GGML_STATUS_SUCCESS;
}

// the NEXT sharded step, started ahead of the host (ahead_launch): the token id and the positions are already on rank 0 (the prep launch in front of this wrote them); the
// hand-over, then the captured graphs and the join.  The cache shards need no refresh: the previous step left them one row short of this one, and this step writes that row.
int tp_ahead_replay(hip_backend_ctx * c) {
    auto & T = g_tp; auto & Q = T.rp;
    if (!Q.valid || T.execs.empty() || T.execs.size() != Q.streams.size()) return CLLM_E_INVALID;
    int rc = tp_hand_over(c, Q.in);
    if (rc == CLLM_OK) rc = tp_launch_graphs(Q.streams, Q.sgpu);
    if (rc == CLLM_OK) rc = tp_join(c);
    cllm_set_device(c->device);
    if (rc != CLLM_OK) return rc;
    for (tp_rank & R : T.r) R.kv_valid = Q.n_kv + 1;
    Q.n_kv += 1; T.steps++; T.last_tp = true;
    return CLLM_OK;
}
#undef TP_TRY
#undef TP_NO
