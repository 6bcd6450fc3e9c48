// fuse_plan.h -- the fusion planner of the ggml module: which nodes of a cgraph become which fused launches.
// Part of ggml-hip.cpp's translation unit: included there, inside its anonymous namespace, after the tensor predicates
// (is_q, f32_dense, ours ...) and the options table.  The planner launches nothing and owns no device memory; decisions that
// need device state (is there a packed copy of these weights?) are taken later, by the walk over the plan.
#pragma once

// ---- node-pattern fusion (decode graphs: a token is ~25 launches per layer node by node, ~5 us each) -------------------------------
// A pattern is fused only if every intermediate it swallows is used by nobody else: the graph-wide use count
// (ggml_node_get_use_count, shared by scheduler splits) must equal the uses found in THIS graph, and the tensor must not be a
// graph output.  All fused launches are bit-identical to the node sequence they replace (same kernels' arithmetic).
//   RMS_NORM -> MUL(weight) -> {MUL_MAT ...}      norm + weight + quantize in every consumer mat-vec's prologue (pro 1)
//   UNARY(SILU) -> MUL(up) -> MUL_MAT             SiLU*up + quantize in the mat-vec's prologue (pro 4)
//   MUL_MAT -> ADD(residual | bias)               epilogue
//   SCALE -> DIAG_MASK_INF -> SOFT_MAX            cllm_op_scale_mask_soft_max
//   {MUL_MAT q, k, v} of a fused attention block      one launch over the packed q|k|v weights (get_pack)
//   {MUL_MAT gate, up} -> SILU -> MUL -> MUL_MAT       one launch over the row-interleaved gate/up weights with the SiLU*up epilogue; the
//                                                      consumer mat-vec then only quantizes (pro 2)
struct fused_mv {
    int pro = 2; const float * px = nullptr; const float * pw = nullptr; float eps = 0.0f; const float * resid = nullptr; float * dst = nullptr;
    const ggml_tensor * resid_t = nullptr;      // the ADD's other operand (a bias when it is a weight leaf)
    int node = -1;                      // the MUL_MAT node
    int ga = -1, gb = -1;               // pro 4: the nodes producing px (gate) and pw (up)
    int group = -1;                     // member of a merged launch (fuse_plan::groups)
    bool alias = false;                 // dst overlaps an input every workgroup reads in its prologue (ggml-alloc re-used a freed parent's block): stage the output
};
struct merge_group {
    int n = 0, member[3] = { -1, -1, -1 };      // entries of mvs, in packed row order
    bool interleave = false;                     // gate/up: SiLU*up epilogue, output = half the rows
    bool bias = false;                           // q|k|v with biases (Qwen2): the three bias vectors are packed too and ride in the epilogue
    int consumer = -1;                           // gate/up: the entry of mvs (pro 4) that reads the activation
    int state = 0;                               // at run time: 0 not reached, 1 launched merged, 2 members launch separately
};
//   ROPE(q) ROPE(k) SET_ROWS(k) CPY(v) MUL_MAT(K,Q) SCALE DIAG_MASK_INF SOFT_MAX MUL_MAT(V,P) PERMUTE CONT
//                                                 the single-token attention block of KVCacheAttention (src/layers.cpp:3044-3123,
//                                                 2499-2561) as cllm_op_rope_kv_attn_decode (level 2: the q/k/v mat-vecs write into
//                                                 module scratch) or, with a RoPE flavour that call does not take (YaRN, frequency
//                                                 factors, partial rotation), the last seven as cllm_op_attn_decode (level 1)
struct fused_attn {
    int level = 0;
    int wq = -1, wk = -1, wv = -1;      // level 2: entries of mvs producing the un-rotated q / k / v
    const float * q = nullptr;          // level 1: the rotated q
    const int32_t * pos = nullptr;      // I32 [1] on the device: the position == cached length - 1
    bool alias = false;                 // level 1: out overlaps the rotated q other heads still read: stage the output
    int nh = 0, nkv = 0, hd = 0, mode = 0;
    float freq_base = 0.0f;
    int64_t n_kv = 0, ML = 0;
    void * k_cache = nullptr, * v_cache = nullptr;
    float * out = nullptr;
};
//   UNARY(SILU) -> MUL                               cllm_op_silu_mul (consumers other than a single-column mat-vec: the expert block of a sparse MoE)
//   RMS_NORM -> MUL(weight)                          cllm_op_rms_norm_mul (where the norm cannot go into its consumers' prologues)
//   GET_ROWS(probs, ids) -> SUM_ROWS -> DIV -> MUL(experts) -> ADD of the slot views (-> ADD residual)
//                                                    cllm_op_moe_combine: the tail of GenericSparseMLP::forward (src/layers.cpp:3792-3872)
//   {MUL_MAT_ID gate, MUL_MAT_ID up} -> UNARY(SILU) -> MUL     one token: cllm_op_mul_mat_id_silu_mul over the per-expert interleaved pack
struct fused_moe { const ggml_tensor * experts = nullptr, * probs = nullptr, * ids = nullptr, * resid = nullptr; int down = -1; /* the MUL_MAT_ID node folded into the launch */ };
//   RMS_NORM -> MUL(weight) -> {MUL_MAT(router) -> SOFT_MAX -> TOP_K, experts}     one token: cllm_op_moe_router (launched at the TOP_K node)
struct moe_router { const ggml_tensor * x = nullptr, * w = nullptr, * gate = nullptr, * xnorm = nullptr, * probs = nullptr; float eps = 0;
                    int itk = -1; std::vector<int> xn_users, out_users; };      // itk: the TOP_K node; who else reads the normalised activation / the probabilities and ids (end nodes behind no-op views)
//   prefill (>= cllm_mul_mat_ex_min_cols() columns): RMS_NORM -> MUL -> {MUL_MAT ...} (norm in the quantizer; further projections of the same activation reuse
//   the act rows), UNARY(SILU) -> MUL -> MUL_MAT (SiLU * up in the quantizer), MUL_MAT -> ADD (residual in the epilogue): cllm_op_mul_mat_ex at the MUL_MAT node
struct pf_mm { int pro = 0; const ggml_tensor * x = nullptr, * w2 = nullptr; float eps = 0; const ggml_tensor * resid = nullptr, * out = nullptr; };
struct moe_gate_up { int mul = -1, gate = -1, up = -1, unary = -1; void * W = nullptr; int router = -1; };      // node indices; W: the pack, resolved before the walk;
                                                                                                                  // router: the block's router folded into this launch (cllm_op_moe_router_gate_up)
//   MUL_MAT(K, Q) SCALE DIAG_MASK_INF SOFT_MAX MUL_MAT(V^T, P)   with more than 32 query rows (the tolerance tier of the MFMA mat-muls):
//                                                    cllm_op_attn_prefill, one flash kernel in place of the V.P node; the scores never reach HBM
struct fused_fa { int ikq = -1, n_past = 0; float scale = 1.0f; bool alias = false; size_t bytes = 0; };   // alias: dst overlaps q (ggml-alloc reuses the dead q block): staged
enum { ALT_NONE = 0, ALT_SILU_MUL = 1 /* src0 is the SiLU */, ALT_RMS_NORM_MUL = 2, ALT_MOE_COMBINE = 3, ALT_MUL_SILU = 4 /* src1 is the SiLU */, ALT_MOE_GATE_UP = 5, ALT_FLASH_PREFILL = 6, ALT_MOE_ROUTER = 7 };
struct fuse_plan {
    std::vector<uint8_t> skip;          // node is produced inside a fused launch (or not needed at all)
    std::vector<uint8_t> alt;           // the node is launched as one of the ALT_* forms
    std::vector<int>     moe;           // ALT_MOE_COMBINE: index into moes; ALT_FLASH_PREFILL: index into fas
    std::vector<fused_fa> fas;
    std::vector<fused_moe> moes;
    std::vector<moe_router> routers;    // ALT_MOE_ROUTER: P.moe[top_k node] indexes them
    std::vector<pf_mm> pfs; std::vector<int> pf;       // prefill mat-muls with a fused prologue / epilogue: pf[MUL_MAT node] indexes pfs
    std::vector<moe_gate_up> gus;       // candidates (P.moe[mul node] indexes them once resolved)
    std::vector<int>     mv;            // index into mvs for MUL_MAT nodes launched fused, else -1
    std::vector<fused_mv> mvs;
    std::vector<int>     sm_src;        // SOFT_MAX nodes: node index of the SCALE feeding the fused scale+mask+soft_max, else -1
    std::vector<int>     attn;          // CONT nodes: index into attns of the fused attention launched in their place, else -1
    std::vector<fused_attn> attns;
    std::vector<merge_group> groups;
};

bool f32_vec(const ggml_tensor * t) { return t && t->type == GGML_TYPE_F32 && t->nb[0] == 4 && t->ne[1] == 1 && t->ne[2] == 1 && t->ne[3] == 1 && ((uintptr_t) t->data & 15) == 0; }
bool overlap(const void * a, size_t na, const void * b, size_t nb) { return (const char *) a < (const char *) b + nb && (const char *) b < (const char *) a + na; }

// planning runs once per graph_compute, before the first launch: flat, allocation-free containers (reused between calls)
struct int_span {
    const int * b, * e;
    const int * begin() const { return b; }
    const int * end() const { return e; }
    int operator[](size_t k) const { return b[k]; }
};
struct user_lists {                 // the consumers of every node, in node order (CSR)
    std::vector<int> start, list;
    int_span operator[](int i) const { return { list.data() + start[i], list.data() + start[i + 1] }; }
};
struct node_index {                 // ggml_tensor * -> position in the graph (open addressing)
    std::vector<const ggml_tensor *> key; std::vector<int> val; size_t mask = 0;
    static size_t h(const void * p) { return (size_t)(((uintptr_t) p >> 4) * 0x9E3779B97F4A7C15ull >> 24); }
    void build(ggml_cgraph * g, int n) {
        size_t cap = 64; while (cap < (size_t) n * 2) cap <<= 1;
        key.assign(cap, nullptr); val.resize(cap); mask = cap - 1;
        for (int i = 0; i < n; i++) { const ggml_tensor * t = ggml_graph_node(g, i); size_t s = h(t) & mask; while (key[s]) s = (s + 1) & mask; key[s] = t; val[s] = i; }
    }
    int operator()(const ggml_tensor * t) const { for (size_t s = h(t) & mask;; s = (s + 1) & mask) { if (key[s] == t) return val[s]; if (!key[s]) return -1; } }
};

void plan_attention(ggml_cgraph * g, fuse_plan & P, const std::vector<int> & local, const std::vector<int> & writer,
                    const user_lists & users, const node_index & find) {
    const int max_level = g_opt.fuse_attn;
    if (max_level <= 0) return;
    const int n = ggml_graph_n_nodes(g);
    auto node = [&](int i) { return ggml_graph_node(g, i); };
    auto only_local = [&](int i, int uses) {
        return i >= 0 && !(node(i)->flags & GGML_TENSOR_FLAG_OUTPUT) && local[i] == uses && ggml_node_get_use_count(g, i) == uses;
    };
    static const int flash_min = cllm_attn_prefill_min_cols();
    // x -> RESHAPE* -> ROPE -> RESHAPE* -> end : returns the ROPE and the node under it; every node of the chain is collected
    auto through_reshapes = [&](const ggml_tensor * t, std::vector<int> & chain) {      // (a VIEW of everything at offset 0 is a reshape too)
        while (t && (t->op == GGML_OP_RESHAPE || (t->op == GGML_OP_VIEW && t->src[0] && t->data == t->src[0]->data && ggml_nelements(t) == ggml_nelements(t->src[0]) &&
                                                   ggml_is_contiguous(t) && ggml_is_contiguous(t->src[0])))) { chain.push_back(find(t)); t = t->src[0]; }
        return t;
    };
    for (int i = 0; i < n; i++) {
        if (P.sm_src[i] < 0) continue;
        const ggml_tensor * sm = node(i), * scn = node(P.sm_src[i]);
        const ggml_tensor * kq = scn->src[0];
        const int ikq = find(kq);
        if (ikq < 0 || kq->op != GGML_OP_MUL_MAT || !only_local(ikq, 1) || !only_local(i, 1)) continue;
        const ggml_tensor * kp = kq->src[0], * qp = kq->src[1];
        if (kp->type == GGML_TYPE_F16 && qp->type == GGML_TYPE_F32 && qp->ne[1] >= flash_min && users[i].end() - users[i].begin() == 1) {      // ---- prefill: the flash kernel
            const int ikqv = users[i][0];
            const ggml_tensor * kqv = node(ikqv), * vv = kqv->src[0];
            const int64_t hd = kp->ne[0], n_kv = kp->ne[1], nkv = kp->ne[2], nh = qp->ne[2], ql = qp->ne[1];
            const int n_past = sm->src[0]->op_params[0];
            auto al16 = [](const ggml_tensor * t) { return (((uintptr_t) t->data | t->nb[1] | t->nb[2] | t->nb[3]) & 15) == 0; };
            if (kqv->op == GGML_OP_MUL_MAT && kqv->src[1] == sm && P.mv[ikqv] < 0 && !P.skip[ikqv] && (hd == 64 || hd == 128) && kp->ne[3] == 1 && qp->ne[3] == 1 && qp->ne[0] == hd &&
                nkv > 0 && nh % nkv == 0 && n_past >= 0 && n_kv == n_past + ql && kp->nb[0] == 2 && qp->nb[0] == 4 && al16(kp) && al16(qp) && al16(kqv) && kqv->type == GGML_TYPE_F32 && kqv->nb[0] == 4 &&
                vv->type == GGML_TYPE_F16 && vv->ne[0] == n_kv && vv->ne[1] == hd && vv->ne[2] == nkv && vv->ne[3] == 1 && vv->nb[0] == 2 && al16(vv) && (int64_t)(vv->nb[1] / 2) >= n_kv &&
                ggml_is_contiguous(kqv) && sm->src[0]->src[0] == scn) {
                fused_fa F; F.ikq = ikq; F.n_past = n_past; memcpy(&F.scale, scn->op_params, 4);
                const bool force_stage = g_opt.force_stage;
                size_t qext = 0;                            // the bytes the (permuted) q view spans
                for (int k = 0; k < 4; k++) qext += (size_t)(qp->ne[k] - 1) * qp->nb[k];
                F.bytes = ggml_nbytes(kqv);
                F.alias = force_stage || overlap(kqv->data, F.bytes, qp->data, qext + 4);
                P.skip[ikq] = P.skip[i] = 1;
                P.alt[ikqv] = ALT_FLASH_PREFILL; P.moe[ikqv] = (int) P.fas.size(); P.fas.push_back(F);
            }
            continue;
        }
        if (kp->type != GGML_TYPE_F16 || qp->type != GGML_TYPE_F32 || qp->op != GGML_OP_PERMUTE) continue;
        const int64_t hd = kp->ne[0], n_kv = kp->ne[1], nkv = kp->ne[2], nh = qp->ne[2];
        if (kp->ne[3] != 1 || qp->ne[0] != hd || qp->ne[1] != 1 || qp->ne[3] != 1 || nkv <= 0 || nh <= 0 || nh % nkv || n_kv < 1) continue;
        const size_t KD = (size_t) hd * nkv;
        if (kp->nb[0] != 2 || kp->nb[1] != KD * 2 || kp->nb[2] != (size_t) hd * 2 || qp->nb[0] != 4 || qp->nb[2] != (size_t) hd * 4) continue;
        float scale; memcpy(&scale, scn->op_params, 4);
        if (scale != 1.0f / sqrtf((float) hd) || sm->src[0]->op_params[0] != (int32_t)(n_kv - 1)) continue;
        // ---- V.P -> PERMUTE -> CONT
        const int ikqv = users[i][0];
        const ggml_tensor * kqv = node(ikqv);
        if (kqv->op != GGML_OP_MUL_MAT || kqv->src[1] != sm || !only_local(ikqv, 1)) continue;
        const ggml_tensor * vv = kqv->src[0];
        if (vv->type != GGML_TYPE_F16 || vv->ne[0] != n_kv || vv->ne[1] != hd || vv->ne[2] != nkv || vv->ne[3] != 1 || vv->nb[0] != 2 || vv->nb[1] % 2) continue;
        const int64_t ML = (int64_t)(vv->nb[1] / 2);
        if (ML < n_kv || vv->nb[2] != (size_t) hd * vv->nb[1] || !cllm_attn_decode_supported((int) nh, (int) nkv, (int) hd, ML)) continue;
        const int iperm = users[ikqv][0];
        const ggml_tensor * perm = node(iperm);
        if (perm->op != GGML_OP_PERMUTE || perm->src[0] != kqv || !only_local(iperm, 1) || perm->ne[0] != hd || perm->ne[1] != nh || perm->ne[2] != 1) continue;
        const int icont = users[iperm][0];
        const ggml_tensor * cont = node(icont);
        if (cont->op != GGML_OP_CONT || cont->src[0] != perm || !f32_dense(cont) || !ggml_is_contiguous(cont) || ((uintptr_t) cont->data & 15)) continue;
        // ---- q: PERMUTE(ROPE(RESHAPE*(q vector), pos))
        const ggml_tensor * qrope = qp->src[0];
        const int iqp = find(qp), iqrope = find(qrope);
        if (qrope->op != GGML_OP_ROPE || iqp < 0 || iqrope < 0 || !only_local(iqp, 1) || !only_local(iqrope, 1)) continue;
        const ggml_tensor * pos = qrope->src[1];
        if (!pos || pos->type != GGML_TYPE_I32 || ggml_nelements(pos) != 1 || !pos->data) continue;
        // ---- the cache writes of this step: K row n_kv - 1 <- RESHAPE*(ROPE(RESHAPE*(k vector), pos)), by SET_ROWS(k_cache, ., pos)
        //      (KVCacheAttention) or by CPY into a view of that row (the sliding-window attention classes); CPY(TRANSPOSE(v vector) -> column n_kv - 1)
        int iset = -1, icpy = -1;
        const char * vcol = (const char *) vv->data + (size_t)(n_kv - 1) * 2, * krow = (const char *) kp->data + (size_t)(n_kv - 1) * KD * 2;
        for (int j = ikq - 1; j >= 0 && j >= ikq - 64 && (iset < 0 || icpy < 0); j--) {
            const ggml_tensor * t = node(j);
            if (iset < 0 && t->op == GGML_OP_SET_ROWS && t->data == kp->data) iset = j;
            if (iset < 0 && t->op == GGML_OP_CPY && t->src[1] && (const char *) t->src[1]->data == krow && (const char *) kp->data != (const char *) vv->data) iset = j;
            if (icpy < 0 && t->op == GGML_OP_CPY && t->src[1] && (const char *) t->src[1]->data == vcol && j != iset) icpy = j;
        }
        if (iset < 0 || icpy < 0 || iset == icpy) continue;
        const ggml_tensor * setr = node(iset), * cpy = node(icpy);
        if (setr->op == GGML_OP_SET_ROWS) {
            if (setr->type != GGML_TYPE_F16 || setr->ne[0] != (int64_t) KD || setr->nb[0] != 2 || setr->nb[1] != KD * 2 || !setr->src[1] || setr->src[1]->data != pos->data ||
                setr->src[1]->type != GGML_TYPE_I32 || ggml_nelements(setr->src[1]) != 1) continue;
        } else {
            const ggml_tensor * kdst = setr->src[1];
            if (kdst->type != GGML_TYPE_F16 || ggml_nelements(kdst) != (int64_t) KD || !ggml_is_contiguous(kdst) || setr->src[0]->type != GGML_TYPE_F32 ||
                ggml_nelements(setr->src[0]) != (int64_t) KD || !ggml_is_contiguous(setr->src[0])) continue;
        }
        const ggml_tensor * vdst = cpy->src[1], * vT = cpy->src[0];
        if (vdst->type != GGML_TYPE_F16 || vdst->ne[0] != 1 || vdst->ne[1] != (int64_t) KD || vdst->nb[1] != (size_t) ML * 2 || vT->type != GGML_TYPE_F32 ||
            vT->op != GGML_OP_TRANSPOSE || vT->ne[0] != 1 || vT->ne[1] != (int64_t) KD || vT->nb[1] != 4) continue;
        std::vector<int> kchain, qchain;
        const ggml_tensor * krope = through_reshapes(setr->src[0], kchain);
        if (!krope || krope->op != GGML_OP_ROPE || !krope->src[1] || krope->src[1]->data != pos->data || ggml_nelements(krope) != (int64_t) KD || krope->ne[0] != hd) continue;
        if (memcmp(krope->op_params + 1, qrope->op_params + 1, 10 * sizeof(int32_t)) || krope->src[2] != qrope->src[2]) continue;
        kchain.push_back(find(krope));
        const ggml_tensor * ks = through_reshapes(krope->src[0], kchain);
        const ggml_tensor * qs = through_reshapes(qrope->src[0], qchain);
        const ggml_tensor * vs = vT->src[0];
        const int iks = find(ks), iqs = find(qs), ivs = find(vs), ivT = find(vT);

        fused_attn A;
        A.pos = (const int32_t *) pos->data; A.nh = (int) nh; A.nkv = (int) nkv; A.hd = (int) hd; A.n_kv = n_kv; A.ML = ML;
        A.k_cache = kp->data; A.v_cache = vv->data; A.out = (float *) cont->data;
        A.mode = qrope->op_params[2]; memcpy(&A.freq_base, qrope->op_params + 5, 4);
        float freq_scale, ext_factor, attn_factor;
        memcpy(&freq_scale, qrope->op_params + 6, 4); memcpy(&ext_factor, qrope->op_params + 7, 4); memcpy(&attn_factor, qrope->op_params + 8, 4);
        bool l2 = max_level >= 2 && (A.mode == 0 || A.mode == 2) && qrope->op_params[1] == hd && freq_scale == 1.0f && ext_factor == 0.0f && attn_factor == 1.0f &&
                  !qrope->src[2] && hd % 4 == 0 && local[iset] == 0 && local[icpy] == 0 && only_local(ivT, 1);
        l2 = l2 && iks >= 0 && iqs >= 0 && ivs >= 0 && only_local(iks, 1) && only_local(iqs, 1) && only_local(ivs, 1) &&
             writer[iks] >= 0 && writer[iqs] >= 0 && writer[ivs] >= 0 && ggml_nelements(ks) == (int64_t) KD && ggml_nelements(vs) == (int64_t) KD && ggml_nelements(qs) == hd * nh;
        for (int j : kchain) l2 = l2 && only_local(j, 1);
        for (int j : qchain) l2 = l2 && only_local(j, 1);
        if (l2) {
            A.level = 2; A.wq = writer[iqs]; A.wk = writer[iks]; A.wv = writer[ivs];
            for (int j : kchain) P.skip[j] = 1;
            for (int j : qchain) P.skip[j] = 1;
            P.skip[iqrope] = P.skip[iset] = P.skip[icpy] = 1;
        } else {
            A.level = 1; A.q = (const float *) qp->data;
        }
        P.skip[ikq] = P.skip[i] = P.skip[ikqv] = 1;         // (SCALE and DIAG_MASK_INF are already swallowed by the soft_max pattern)
        P.attn[icont] = (int) P.attns.size(); P.attns.push_back(A);
    }
}

fuse_plan make_plan(ggml_cgraph * g) {
    const int n = ggml_graph_n_nodes(g);
    fuse_plan P; P.skip.assign(n, 0); P.mv.assign(n, -1); P.sm_src.assign(n, -1); P.attn.assign(n, -1); P.alt.assign(n, ALT_NONE); P.moe.assign(n, -1); P.pf.assign(n, -1);
    if (g_opt.no_fuse || n < 8) return P;
    std::vector<int> local(n, 0), writer(n, -1);        // writer[i]: entry of mvs whose launch produces node i
    static thread_local node_index find;
    static thread_local user_lists users;
    static thread_local std::vector<int> edges;
    find.build(g, n);
    // uses inside this graph (views count as uses of their source, exactly like ggml's use counts)
    edges.clear();
    for (int j = 0; j < n; j++) {
        const ggml_tensor * t = ggml_graph_node(g, j);
        for (int k = 0; k < GGML_MAX_SRC; k++) if (t->src[k]) { const int i = find(t->src[k]); if (i >= 0 && i < j) { local[i]++; edges.push_back(i); edges.push_back(j); } }
    }
    users.start.assign(n + 1, 0);
    for (int i = 0; i < n; i++) users.start[i + 1] = users.start[i] + local[i];
    users.list.resize(edges.size() / 2);
    {
        std::vector<int> fill(users.start.begin(), users.start.end() - 1);
        for (size_t e = 0; e < edges.size(); e += 2) users.list[fill[edges[e]]++] = edges[e + 1];      // edges are in consumer order: so is every list
    }
    auto only_local = [&](int i, int uses) {
        const ggml_tensor * t = ggml_graph_node(g, i);
        return !(t->flags & GGML_TENSOR_FLAG_OUTPUT) && local[i] == uses && ggml_node_get_use_count(g, i) == uses;
    };
    auto node_of = [&](const ggml_tensor * t, int before) { for (int i = before - 1; i >= 0 && i >= before - 64; i--) if (ggml_graph_node(g, i) == t) return i; return -1; };
    // a single-column quantized MUL_MAT the decode mat-vec takes; row length: 16384 with the norm prologue, 32768 with the others (gemv_decode.hip)
    auto mv_ok = [&](const ggml_tensor * mm, int64_t kmax = 32768) {
        const ggml_tensor * w = mm->src[0], * x = mm->src[1];
        return mm->op == GGML_OP_MUL_MAT && is_q(w->type) && w->ne[2] == 1 && w->ne[3] == 1 && w->nb[1] == ggml_row_size(w->type, w->ne[0]) && ((uintptr_t) w->data & 15) == 0 &&
               x->type == GGML_TYPE_F32 && x->ne[1] == 1 && x->ne[2] == 1 && x->ne[3] == 1 && f32_vec(mm) &&
               w->ne[0] <= kmax && (uint64_t) w->ne[1] * w->nb[1] < (1ull << 32);
    };
    for (int i = 0; i < n; i++) {
        ggml_tensor * t = ggml_graph_node(g, i);
        // ---- RMS_NORM -> MUL(weight) -> mat-vecs
        if (t->op == GGML_OP_MUL && t->src[0] && t->src[0]->op == GGML_OP_RMS_NORM && f32_vec(t) && f32_vec(t->src[0]->src[0]) && f32_vec(t->src[1]) &&
            t->src[1]->ne[0] == t->ne[0] && t->ne[0] % 256 == 0) {
            const int r = node_of(t->src[0], i);
            bool ok = r >= 0 && only_local(r, 1) && only_local(i, local[i]) && local[i] > 0;
            for (int j : users[i]) { const ggml_tensor * c = ggml_graph_node(g, j); ok = ok && mv_ok(c, 16384) && c->src[1] == t; }
            if (ok) {
                float eps; memcpy(&eps, t->src[0]->op_params, 4);
                for (int j : users[i]) {
                    fused_mv f; f.pro = 1; f.px = (const float *) t->src[0]->src[0]->data; f.pw = (const float *) t->src[1]->data; f.eps = eps; f.dst = (float *) ggml_graph_node(g, j)->data; f.node = j;
                    P.mv[j] = writer[j] = (int) P.mvs.size(); P.mvs.push_back(f);
                }
                P.skip[r] = P.skip[i] = 1;
            }
        }
        // ---- UNARY(SILU) -> MUL(up) -> mat-vec
        if (t->op == GGML_OP_MUL && t->src[0] && t->src[0]->op == GGML_OP_UNARY && ggml_get_unary_op(t->src[0]) == GGML_UNARY_OP_SILU && f32_vec(t) && f32_vec(t->src[0]->src[0]) &&
            f32_vec(t->src[1]) && t->src[1]->ne[0] == t->ne[0] && local[i] == 1) {
            const int u = node_of(t->src[0], i), j = users[i][0];
            const ggml_tensor * c = ggml_graph_node(g, j);
            if (u >= 0 && only_local(u, 1) && only_local(i, 1) && mv_ok(c) && c->src[1] == t && t->ne[0] % 8 == 0 && c->src[0]->ne[0] <= 32768) {
                fused_mv f; f.pro = 4; f.px = (const float *) t->src[0]->src[0]->data; f.pw = (const float *) t->src[1]->data; f.dst = (float *) c->data;
                f.node = j; f.ga = find(t->src[0]->src[0]); f.gb = find(t->src[1]);
                P.mv[j] = writer[j] = (int) P.mvs.size(); P.mvs.push_back(f);
                P.skip[u] = P.skip[i] = 1;
            }
        }
        // ---- SCALE -> DIAG_MASK_INF -> SOFT_MAX (no mask tensor, no ALiBi)
        if (t->op == GGML_OP_SOFT_MAX && !t->src[1] && t->src[0]->op == GGML_OP_DIAG_MASK_INF && t->src[0]->src[0]->op == GGML_OP_SCALE) {
            const int dm = node_of(t->src[0], i), sc = dm >= 0 ? node_of(t->src[0]->src[0], dm) : -1;
            float s1, mb, bias; memcpy(&s1, t->op_params, 4); memcpy(&mb, (const float *) t->op_params + 1, 4);
            if (sc >= 0) memcpy(&bias, (const float *) ggml_graph_node(g, sc)->op_params + 1, 4);
            if (sc >= 0 && only_local(dm, 1) && only_local(sc, 1) && s1 == 1.0f && mb == 0.0f && bias == 0.0f) { P.sm_src[i] = sc; P.skip[dm] = P.skip[sc] = 1; }
        }
    }
    // ---- mat-vec -> ADD: after the prologue patterns, so that it composes with them
    for (int i = 0; i < n; i++) {
        ggml_tensor * a = ggml_graph_node(g, i);
        if (a->op != GGML_OP_ADD || !f32_vec(a)) continue;
        for (int side = 0; side < 2; side++) {
            const ggml_tensor * mm = a->src[side], * r = a->src[1 - side];
            if (!mm || mm->op != GGML_OP_MUL_MAT || !mv_ok(mm) || !f32_vec(r) || r->ne[0] != a->ne[0]) continue;
            const int j = node_of(mm, i);
            if (j < 0 || !only_local(j, 1) || P.skip[j]) continue;
            if (P.mv[j] < 0) { fused_mv f; f.pro = 2; f.px = (const float *) mm->src[1]->data; f.node = j; P.mv[j] = (int) P.mvs.size(); P.mvs.push_back(f); }
            fused_mv & f = P.mvs[P.mv[j]];
            const size_t kbytes = (size_t) mm->src[0]->ne[0] * 4, nbytes = (size_t) a->ne[0] * 4;
            if (overlap(a->data, nbytes, f.px, kbytes) || (f.pw && overlap(a->data, nbytes, f.pw, kbytes))) { if (f.pro == 2 && !f.resid && !f.dst) { P.mvs.pop_back(); P.mv[j] = -1; } continue; }
            f.resid = (const float *) r->data; f.resid_t = r; f.dst = (float *) a->data;
            P.skip[i] = 1;
            writer[j] = -1; writer[i] = P.mv[j];
            break;
        }
    }
    // ---- prefill: the same three patterns around a many-column quantized MUL_MAT (cllm_op_mul_mat_ex; the runner's prefill has them too)
    const bool no_pf = g_opt.no_prefill_fuse;
    static const int pf_min = cllm_mul_mat_ex_min_cols();
    auto pf_ok = [&](const ggml_tensor * mm) {
        if (mm->op != GGML_OP_MUL_MAT) return false;
        const ggml_tensor * w = mm->src[0], * x = mm->src[1];
        const uintptr_t wal = (uintptr_t) wtype_row_align((int) w->type) - 1;       // csrc/types.def: what cllm_op_mul_mat_ex demands of the rows
        return is_q(w->type) && w->ne[2] == 1 && w->ne[3] == 1 && w->nb[1] == ggml_row_size(w->type, w->ne[0]) && !((uintptr_t) w->data & wal) && !(w->nb[1] & wal) &&
               x->type == GGML_TYPE_F32 && x->ne[2] == 1 && x->ne[3] == 1 && x->ne[1] >= pf_min && x->ne[1] <= 65535 && x->nb[0] == 4 && x->nb[1] % 16 == 0 && !((uintptr_t) x->data & 15) &&
               mm->type == GGML_TYPE_F32 && mm->nb[0] == 4 && mm->nb[1] % 4 == 0 && mm->ne[2] == 1 && mm->ne[3] == 1;
    };
    auto act_class = [](ggml_type t) { return act_kind_of((int) t); };      // the act rows two projections can share (every user passed pf_ok: tuned types)
    auto uses_wdata = [](const ggml_tensor * t) { return t->op == GGML_OP_MUL_MAT || t->op == GGML_OP_MUL_MAT_ID || t->op == GGML_OP_FLASH_ATTN_EXT; };
    if (!no_pf) for (int i = 0; i < n; i++) {
        ggml_tensor * t = ggml_graph_node(g, i);
        if (P.skip[i] || t->op != GGML_OP_MUL || t->type != GGML_TYPE_F32 || t->ne[1] < pf_min || t->ne[2] != 1 || t->ne[3] != 1 || !ggml_is_contiguous(t)) continue;
        const ggml_tensor * a = t->src[0], * b = t->src[1];
        // RMS_NORM -> MUL(weight vector) -> projections
        const int ir = find(a);
        if (a->op == GGML_OP_RMS_NORM && ir >= 0 && !P.skip[ir] && only_local(ir, 1) && only_local(i, local[i]) && local[i] > 0 && a->src[0]->type == GGML_TYPE_F32 &&
            ggml_is_contiguous(a->src[0]) && !((uintptr_t) a->src[0]->data & 15) && t->ne[0] % 4 == 0 && t->ne[0] <= 16384 &&
            b->type == GGML_TYPE_F32 && ggml_is_contiguous(b) && ggml_nelements(b) == t->ne[0] && !((uintptr_t) b->data & 15)) {
            bool ok = true;
            for (int j : users[i]) { const ggml_tensor * c = ggml_graph_node(g, j); ok = ok && pf_ok(c) && c->src[1] == t && P.pf[j] < 0 && !P.skip[j]; }
            if (!ok) continue;
            int prev = -1;
            for (int j : users[i]) {
                pf_mm F; F.pro = 1; F.x = a->src[0]; F.w2 = b; memcpy(&F.eps, a->op_params, 4);
                if (prev >= 0 && act_class(ggml_graph_node(g, j)->src[0]->type) == act_class(ggml_graph_node(g, prev)->src[0]->type)) {
                    bool clean = true;                 // nothing between the two projections may touch the module's act scratch
                    for (int k = prev + 1; k < j; k++) clean = clean && !uses_wdata(ggml_graph_node(g, k));
                    if (clean) F.pro = 5;
                }
                P.pf[j] = (int) P.pfs.size(); P.pfs.push_back(F);
                prev = j;
            }
            P.skip[ir] = P.skip[i] = 1;
            continue;
        }
        // UNARY(SILU)(gate) -> MUL(up) -> MUL_MAT
        for (int side = 0; side < 2; side++) {
            const ggml_tensor * u = side ? b : a, * o = side ? a : b;
            const int iu = find(u);
            if (u->op != GGML_OP_UNARY || ggml_get_unary_op(u) != GGML_UNARY_OP_SILU || iu < 0 || P.skip[iu] || !only_local(iu, 1) || !only_local(i, 1)) continue;
            const int j = users[i][0];
            const ggml_tensor * c = ggml_graph_node(g, j), * gate = u->src[0];
            if (!pf_ok(c) || c->src[1] != t || P.pf[j] >= 0 || P.skip[j] || !ggml_are_same_shape(gate, t) || !ggml_are_same_shape(o, t) || gate->type != GGML_TYPE_F32 || o->type != GGML_TYPE_F32 ||
                !ggml_is_contiguous(gate) || !ggml_is_contiguous(o) || ((uintptr_t) gate->data & 15) || ((uintptr_t) o->data & 15) || t->ne[0] % 4) continue;
            pf_mm F; F.pro = 4; F.x = gate; F.w2 = o;
            P.pf[j] = (int) P.pfs.size(); P.pfs.push_back(F);
            P.skip[iu] = P.skip[i] = 1;
            break;
        }
    }
    // MUL_MAT -> ADD(residual): the ADD directly follows (only views in between: its destination is then not the live memory of anything that still runs)
    if (!no_pf) for (int i = 0; i < n; i++) {
        ggml_tensor * ad = ggml_graph_node(g, i);
        if (P.skip[i] || ad->op != GGML_OP_ADD || ad->type != GGML_TYPE_F32 || !ggml_is_contiguous(ad)) continue;
        for (int side = 0; side < 2; side++) {
            const ggml_tensor * mm = ad->src[side], * r = ad->src[1 - side];
            const int j = mm ? find(mm) : -1;
            if (j < 0 || j >= i || !pf_ok(mm) || P.skip[j] || !only_local(j, 1) || !r || r->type != GGML_TYPE_F32 || !ggml_are_same_shape(r, ad) || !ggml_are_same_shape(mm, ad) || !ggml_is_contiguous(r) ||
                !ggml_is_contiguous(mm)) continue;
            bool adjacent = true;
            for (int k = j + 1; k < i; k++) { const ggml_op op = ggml_graph_node(g, k)->op; adjacent = adjacent && (op == GGML_OP_RESHAPE || op == GGML_OP_VIEW || op == GGML_OP_PERMUTE || op == GGML_OP_TRANSPOSE); }
            if (!adjacent || (ad->data != r->data && overlap(ad->data, ggml_nbytes(ad), r->data, ggml_nbytes(r)))) continue;
            if (P.pf[j] < 0) { pf_mm F; F.pro = 0; F.x = mm->src[1]; P.pf[j] = (int) P.pfs.size(); P.pfs.push_back(F); }
            P.pfs[P.pf[j]].resid = r; P.pfs[P.pf[j]].out = ad;
            P.skip[i] = 1;
            break;
        }
    }
    plan_attention(g, P, local, writer, users, find);
    // ---- merged launches over packed weights (the decision whether a packed copy exists is taken at run time: get_pack)
    auto is_bias = [&](const fused_mv & f) {     // the epilogue operand is a weight vector of the projection's length: never an activation
        const ggml_tensor * w = ggml_graph_node(g, f.node)->src[0];
        return f.resid_t && f.resid_t->op == GGML_OP_NONE && ours(f.resid_t) && f.resid_t->type == GGML_TYPE_F32 && ggml_is_contiguous(f.resid_t) &&
               ggml_nelements(f.resid_t) == w->ne[1] && ((uintptr_t) f.resid_t->data & 15) == 0;
    };
    auto same_input = [&](const fused_mv & a, const fused_mv & b, bool with_bias) {
        const ggml_tensor * wa = ggml_graph_node(g, a.node)->src[0], * wb = ggml_graph_node(g, b.node)->src[0];
        const bool epi_ok = with_bias ? (is_bias(a) && is_bias(b)) : (!a.resid && !b.resid);
        return a.pro == 1 && b.pro == 1 && a.px == b.px && a.pw == b.pw && a.eps == b.eps && epi_ok && a.group < 0 && b.group < 0 && !a.alias && !b.alias &&
               wa->type == wb->type && wa->ne[0] == wb->ne[0] && wa->nb[1] == wb->nb[1];
    };
    for (const fused_attn & A : P.attns) {
        if (A.level != 2 || A.wq == A.wk || A.wq == A.wv || A.wk == A.wv) continue;
        const bool with_bias = P.mvs[A.wq].resid != nullptr;
        if (!same_input(P.mvs[A.wq], P.mvs[A.wk], with_bias) || !same_input(P.mvs[A.wq], P.mvs[A.wv], with_bias)) continue;
        merge_group G; G.n = 3; G.member[0] = A.wq; G.member[1] = A.wk; G.member[2] = A.wv; G.bias = with_bias;
        for (int k = 0; k < 3; k++) P.mvs[G.member[k]].group = (int) P.groups.size();
        P.groups.push_back(G);
    }
    for (size_t m = 0; m < P.mvs.size(); m++) {
        const fused_mv & d = P.mvs[m];
        if (d.pro != 4 || d.ga < 0 || d.gb < 0 || d.ga == d.gb || P.mv[d.ga] < 0 || P.mv[d.gb] < 0 || P.skip[d.ga] || P.skip[d.gb]) continue;
        const fused_mv & a = P.mvs[P.mv[d.ga]], & b = P.mvs[P.mv[d.gb]];
        const ggml_tensor * ta = ggml_graph_node(g, d.ga), * tb = ggml_graph_node(g, d.gb);
        if (!same_input(a, b, false) || a.dst != (float *) ta->data || b.dst != (float *) tb->data || !only_local(d.ga, 1) || !only_local(d.gb, 1)) continue;
        const int64_t F = ta->ne[0];
        if (tb->ne[0] != F || F % 8 || ta->src[0]->ne[1] != F || tb->src[0]->ne[1] != F) continue;
        merge_group G; G.n = 2; G.member[0] = P.mv[d.ga]; G.member[1] = P.mv[d.gb]; G.interleave = true; G.consumer = (int) m;
        P.mvs[G.member[0]].group = P.mvs[G.member[1]].group = (int) P.groups.size();
        P.groups.push_back(G);
    }
    for (int j = 0; j < n; j++) if (P.mv[j] >= 0 && !P.mvs[P.mv[j]].dst) P.mvs[P.mv[j]].dst = (float *) ggml_graph_node(g, j)->data;
    // A fused mat-vec has no grid-wide barrier between its prologue (EVERY workgroup reads all of px / pw) and the first stores of dst.
    // ggml-alloc allocates a node before it frees the node's parents, but the tensors a fused launch swallows (the norm's input is not one of
    // them; `up` of SILU->MUL(up)->MUL_MAT, the normalised activation ...) may already be free when dst is placed -- so dst can land on an
    // input.  Such launches write to module scratch and are copied into place afterwards (graph_compute); an in-place residual (dst == resid)
    // is fine: every element is read and written by the same lane.
    const bool force_stage = g_opt.force_stage;      // (tests: take the staged path everywhere)
    for (fused_mv & f : P.mvs) {
        if (f.node < 0 || !f.dst) continue;
        const ggml_tensor * w = ggml_graph_node(g, f.node)->src[0];
        const size_t nb = (size_t) w->ne[1] * 4, kb = (size_t) w->ne[0] * 4;
        f.alias = force_stage || (f.px && overlap(f.dst, nb, f.px, kb)) || (f.pw && overlap(f.dst, nb, f.pw, kb));
    }
    for (fused_attn & A : P.attns) if (A.level == 1) A.alias = force_stage || overlap(A.out, (size_t) A.nh * A.hd * 4, A.q, (size_t) A.nh * A.hd * 4);
    // ---- what the patterns above left: element-wise pairs and the tail of a sparse-MoE block
    auto strip = [&](const ggml_tensor * t) { while (t && t->op == GGML_OP_RESHAPE) t = t->src[0]; return t; };
    auto all_once = [&](const ggml_tensor * from, const ggml_tensor * to) {      // the RESHAPE chain from `from` down to (excluding) `to`: every node used once
        for (const ggml_tensor * t = from; t && t != to; t = t->src[0]) { if (t->op != GGML_OP_RESHAPE || !only_local(find(t), 1)) return false; }
        return true;
    };
    for (int i = 0; i < n; i++) {
        ggml_tensor * t = ggml_graph_node(g, i);
        if (P.skip[i] || t->op != GGML_OP_MUL || t->type != GGML_TYPE_F32) continue;
        const ggml_tensor * a = t->src[0], * b = t->src[1];
        // UNARY(SILU) on either side, same shape, dense
        for (int side = 0; side < 2; side++) {
            const ggml_tensor * u = side ? b : a, * o = side ? a : b;
            const int iu = find(u);
            if (u->op == GGML_OP_UNARY && ggml_get_unary_op(u) == GGML_UNARY_OP_SILU && iu >= 0 && !P.skip[iu] && only_local(iu, 1) && ggml_are_same_shape(u, o) &&
                ggml_are_same_shape(u, t) && f32_dense(u->src[0]) && f32_dense(o) && f32_dense(t) && ggml_is_contiguous(u->src[0]) && ggml_is_contiguous(o) && ggml_is_contiguous(t)) {
                P.alt[i] = side ? ALT_MUL_SILU : ALT_SILU_MUL; P.skip[iu] = 1;
                // both operands straight from one-token MUL_MAT_IDs over the same activation and ids: candidate for the merged expert launch
                const ggml_tensor * gm = u->src[0], * um = o;
                const int igm = find(gm), ium = find(um);
                if (gm->op == GGML_OP_MUL_MAT_ID && um->op == GGML_OP_MUL_MAT_ID && igm >= 0 && ium >= 0 && only_local(igm, 1) && only_local(ium, 1) &&
                    gm->src[1] == um->src[1] && gm->src[2] == um->src[2] && gm->src[2]->ne[1] == 1 && gm->src[2]->nb[0] == 4 &&
                    gm->src[0]->type == um->src[0]->type && is_q(gm->src[0]->type) && ggml_are_same_shape(gm->src[0], um->src[0]) && gm->src[0]->nb[1] == um->src[0]->nb[1] &&
                    gm->src[0]->ne[1] % 8 == 0 && gm->src[0]->ne[0] <= 32768 && gm->src[1]->nb[0] == 4 && gm->src[1]->nb[1] % 16 == 0 && ((uintptr_t) gm->src[1]->data & 15) == 0) {
                    moe_gate_up G; G.mul = i; G.gate = igm; G.up = ium; G.unary = iu;
                    P.gus.push_back(G);
                }
                break;
            }
        }
        if (P.alt[i]) continue;
        // RMS_NORM -> MUL(weight vector)
        const int ir = find(a);
        if (a->op == GGML_OP_RMS_NORM && ir >= 0 && !P.skip[ir] && only_local(ir, 1) && f32_dense(a->src[0]) && ggml_is_contiguous(a->src[0]) && ggml_is_contiguous(t) &&
            b->type == GGML_TYPE_F32 && ggml_is_contiguous(b) && ggml_nelements(b) == t->ne[0] && b->ne[0] == t->ne[0]) {
            // one token, and among the consumers a small router mat-vec -> SOFT_MAX -> TOP_K: the whole head of the sparse-MoE block in one launch
            int imm = -1, ism = -1, itk = -1;
            if (ggml_nelements(t) == t->ne[0] && t->ne[0] % 4 == 0 && !(((uintptr_t) t->data | (uintptr_t) a->src[0]->data | (uintptr_t) b->data) & 15) &&
                (t->data == a->src[0]->data || !overlap(t->data, (size_t) t->ne[0] * 4, a->src[0]->data, (size_t) t->ne[0] * 4)))
                for (int u : users[i]) {
                    const ggml_tensor * c = ggml_graph_node(g, u);
                    if (c->op == GGML_OP_MUL_MAT && c->src[1] == t && mv_ok(c, 16384) && c->src[0]->ne[1] <= 64 && P.mv[u] < 0 && !P.skip[u] && only_local(u, 1)) { imm = u; break; }
                }
            if (imm >= 0) {
                const int u = users[imm][0];
                const ggml_tensor * sm = ggml_graph_node(g, u);
                float s1, mb; memcpy(&s1, sm->op_params, 4); memcpy(&mb, (const float *) sm->op_params + 1, 4);
                if (sm->op == GGML_OP_SOFT_MAX && !sm->src[1] && sm->src[0] == ggml_graph_node(g, imm) && s1 == 1.0f && mb == 0.0f && f32_vec(sm) && !P.skip[u] && P.sm_src[u] < 0 &&
                    !(sm->flags & GGML_TENSOR_FLAG_OUTPUT)) ism = u;
            }
            if (ism >= 0) {
                int cnt = 0;
                for (int u : users[ism]) { const ggml_tensor * c = ggml_graph_node(g, u); if (c->op == GGML_OP_TOP_K && c->src[0] == ggml_graph_node(g, ism)) { itk = u; cnt++; } }
                const ggml_tensor * tk = itk >= 0 ? ggml_graph_node(g, itk) : nullptr;
                if (cnt != 1 || tk->type != GGML_TYPE_I32 || tk->nb[0] != 4 || ggml_nelements(tk) != tk->ne[0] || tk->ne[0] > ggml_graph_node(g, ism)->ne[0] || P.skip[itk]) itk = -1;
            }
            if (itk >= 0) {
                // everything else that reads the normalised activation or the probabilities must run after the launch (which stands at the TOP_K node)
                std::function<bool(int)> later = [&](int j) {
                    for (int u : users[j]) {
                        if (u == imm || u == ism || u == itk) continue;
                        const ggml_tensor * c = ggml_graph_node(g, u);
                        const bool noop = c->op == GGML_OP_RESHAPE || c->op == GGML_OP_VIEW || c->op == GGML_OP_PERMUTE || c->op == GGML_OP_TRANSPOSE;
                        if (noop ? !later(u) : u < itk) return false;
                    }
                    return true;
                };
                if (later(i) && later(ism)) {
                    moe_router R; R.x = a->src[0]; R.w = b; R.gate = ggml_graph_node(g, imm)->src[0]; R.xnorm = t; R.probs = ggml_graph_node(g, ism);
                    memcpy(&R.eps, a->op_params, 4);
                    R.itk = itk;
                    std::function<void(int, std::vector<int> &)> ends = [&](int j, std::vector<int> & out) {      // the end consumers of node j behind no-op views
                        for (int u : users[j]) {
                            if (u == imm || u == ism || u == itk) continue;
                            const ggml_tensor * c = ggml_graph_node(g, u);
                            if (c->op == GGML_OP_RESHAPE || c->op == GGML_OP_VIEW || c->op == GGML_OP_PERMUTE || c->op == GGML_OP_TRANSPOSE) ends(u, out); else out.push_back(u);
                        }
                    };
                    ends(i, R.xn_users); ends(ism, R.out_users); ends(itk, R.out_users);
                    P.skip[ir] = P.skip[i] = P.skip[imm] = P.skip[ism] = 1;
                    P.alt[itk] = ALT_MOE_ROUTER; P.moe[itk] = (int) P.routers.size(); P.routers.push_back(R);
                    continue;
                }
            }
            P.alt[i] = ALT_RMS_NORM_MUL; P.skip[ir] = 1;
            continue;
        }
        // experts [H, k, T] * weights [1, k, T], weights = RESHAPE(DIV(RESHAPE(GET_ROWS(RESHAPE(probs), ids)), SUM_ROWS(same)))
        if (a->ne[3] != 1 || b->ne[0] != 1 || b->ne[1] != a->ne[1] || b->ne[2] != a->ne[2] || !f32_dense(a) || !ggml_is_contiguous(a) || !ggml_is_contiguous(t)) continue;
        const int64_t H = a->ne[0], k = a->ne[1], T = a->ne[2];
        const ggml_tensor * dv = strip(b);
        if (!dv || dv->op != GGML_OP_DIV || !all_once(b, dv) || !only_local(find(dv), 1)) continue;
        const ggml_tensor * wr = dv->src[0], * sr = dv->src[1];
        const int iwr = find(wr), isr = find(sr);
        if (sr->op != GGML_OP_SUM_ROWS || sr->src[0] != wr || !only_local(isr, 1) || wr->op != GGML_OP_RESHAPE || iwr < 0 || local[iwr] != 2 || ggml_node_get_use_count(g, iwr) != 2 ||
            wr->ne[0] != k || wr->ne[1] != T) continue;
        const ggml_tensor * gr = wr->src[0];
        const int igr = find(gr);
        if (gr->op != GGML_OP_GET_ROWS || !only_local(igr, 1) || gr->ne[0] != 1) continue;
        const ggml_tensor * probs = strip(gr->src[0]), * ids = gr->src[1];
        if (!probs || probs->type != GGML_TYPE_F32 || !ggml_is_contiguous(probs) || probs->ne[1] != T || ggml_nelements(probs) != probs->ne[0] * T ||
            ids->type != GGML_TYPE_I32 || ids->ne[0] != k || ids->ne[1] != T || ids->nb[0] != 4) continue;
        // the k slot views and the ADD chain
        if (local[i] != (int) k || ggml_node_get_use_count(g, i) != (int) k || (t->flags & GGML_TENSOR_FLAG_OUTPUT) || k < 1 || k > 64) continue;
        std::vector<int> views((size_t) k, -1);
        bool ok = true;
        for (int u : users[i]) {
            const ggml_tensor * v = ggml_graph_node(g, u);
            const size_t off = (size_t)((const char *) v->data - (const char *) t->data);
            if (v->op != GGML_OP_VIEW || v->src[0] != t || v->ne[0] != H || v->ne[1] != T || v->ne[2] != 1 || v->nb[1] != t->nb[2] || off % t->nb[1] || off / t->nb[1] >= (size_t) k ||
                views[off / t->nb[1]] >= 0 || !only_local(u, 1)) { ok = false; break; }
            views[off / t->nb[1]] = u;
        }
        if (!ok) continue;
        int cur = views[0];
        std::vector<int> adds;
        for (int64_t j = 1; j < k && ok; j++) {
            const int ia = users[cur][0];
            const ggml_tensor * ad = ggml_graph_node(g, ia);
            ok = ad->op == GGML_OP_ADD && ad->src[0] == ggml_graph_node(g, cur) && ad->src[1] == ggml_graph_node(g, views[(size_t) j]) && users[views[(size_t) j]][0] == ia &&
                 f32_dense(ad) && ggml_is_contiguous(ad) && (j == k - 1 || only_local(ia, 1));
            adds.push_back(ia); cur = ia;
        }
        if (!ok || k < 2) continue;
        fused_moe M; M.experts = a; M.probs = probs; M.ids = ids;
        int fin = cur;
        // every thread of k_moe_combine reads its element of all k slots (and of the residual), then writes its element of dst: dst may BE slot 0 of
        // a one-token experts tensor or the residual (ggml-alloc computes these ADDs in place), but must not overlap them any other way
        auto dst_ok = [&](const ggml_tensor * out, const ggml_tensor * resid) {
            const char * dp = (const char *) out->data;
            const size_t nb = (size_t)(H * T) * 4;
            if (overlap(dp, nb, a->data, ggml_nbytes(a)) && !(T == 1 && dp == (const char *) a->data)) return false;
            return !resid || dp == (const char *) resid->data || !overlap(dp, nb, resid->data, nb);
        };
        if (only_local(cur, 1)) {             // ... -> ADD(moe_out, residual)
            const int ia = users[cur][0];
            const ggml_tensor * ad = ggml_graph_node(g, ia);
            if (ad->op == GGML_OP_ADD && !P.skip[ia] && ad->src[0] == ggml_graph_node(g, cur) && f32_dense(ad->src[1]) && ggml_is_contiguous(ad->src[1]) &&
                ad->src[1]->ne[0] == H && ggml_nelements(ad->src[1]) == H * T && ggml_is_contiguous(ad) && dst_ok(ad, ad->src[1])) { M.resid = ad->src[1]; fin = ia; }
        }
        if (!M.resid && !dst_ok(ggml_graph_node(g, cur), nullptr)) continue;
        {   // the experts are the down projection's MUL_MAT_ID of one token over two slots: mat-vecs and tail in one launch (cllm_op_mul_mat_id_combine)
            const int ia = find(a);
            const ggml_tensor * out = ggml_graph_node(g, fin), * w = a->src[0], * x = a->src[1];
            if (!g_opt.no_moe_down_fuse && a->op == GGML_OP_MUL_MAT_ID && ia >= 0 && !P.skip[ia] && only_local(ia, 1) && k == 2 && T == 1 && a->src[2] == ids && is_q(w->type) && w->ne[3] == 1 &&
                w->nb[1] == ggml_row_size(w->type, w->ne[0]) && w->nb[2] % 16 == 0 && ((uintptr_t) w->data & 15) == 0 && w->ne[0] <= 32768 && (uint64_t) w->ne[1] * w->nb[1] < (1ull << 32) &&
                x->type == GGML_TYPE_F32 && x->ne[1] == 2 && x->ne[2] == 1 && x->ne[3] == 1 && x->nb[0] == 4 && x->nb[1] % 16 == 0 && ((uintptr_t) x->data & 15) == 0 &&
                probs->ne[0] == w->ne[2] && ggml_nelements(probs) == probs->ne[0] &&
                !overlap(out->data, (size_t) H * 4, x->data, ggml_nbytes(x)) && !overlap(out->data, (size_t) H * 4, probs->data, ggml_nbytes(probs)) &&
                !overlap(out->data, (size_t) H * 4, ids->data, ggml_nbytes(ids))) { M.down = ia; P.skip[ia] = 1; }
        }
        for (const ggml_tensor * r = b; r != dv; r = r->src[0]) P.skip[find(r)] = 1;
        P.skip[find(dv)] = P.skip[isr] = P.skip[iwr] = P.skip[igr] = 1;
        for (const ggml_tensor * r = gr->src[0]; r != probs; r = r->src[0]) if (find(r) >= 0) P.skip[find(r)] = 1;       // (RESHAPEs: no launches anyway)
        P.skip[i] = 1;
        for (int ia : adds) P.skip[ia] = 1;
        if (M.resid) P.skip[cur] = 1;
        P.skip[fin] = 0; P.alt[fin] = ALT_MOE_COMBINE; P.moe[fin] = (int) P.moes.size(); P.moes.push_back(M);
    }
    return P;
}
