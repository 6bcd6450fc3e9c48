// ggml-hip.cpp -- the reference-side binding: a ggml backend MODULE ("libggml-hip.so") over the C ABI of
// libchatllm_hip.so (include/chatllm_hip.h).  This is the drop-in boundary of SURVEY.md 8b:
//   * exports  ggml_backend_reg_t ggml_backend_init(void)            (ggml/src/ggml-backend-impl.h:206-251)
//   * implements the five vtables reg / device / buffer_type / buffer / backend   (ggml-backend-impl.h:11-251)
//   * is found by the unmodified chatllm.cpp host through ggml_backend_load_all_from_path(), slot "hip", BEFORE the
//     CPU module (ggml/src/ggml-backend-reg.cpp:545-575), so CPU stays the last device (src/backend.cpp:727-737).
// It is compiled against the reference's headers WHERE THEY LIE (/root/reference/ggml/include, ggml/src) -- nothing is
// copied -- and contains no kernels: graph_compute() walks the cgraph and maps every node 1:1 onto a cllm_op_* call.
// Unsupported nodes are declined in supports_op() so that ggml's scheduler places them on the CPU backend.
#include "ggml.h"
#include "ggml-backend.h"
#include "ggml-backend-impl.h"
#include "ggml-impl.h"          // ggml_node_get_use_count: the graph-wide use counts the fusion pass relies on

#include "../../include/chatllm_hip.h"
#include "../csrc/types.h"       // what a tensor type is: is_quant_type, is_kq_type (csrc/types.def)

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>
#include <functional>

#define HIPB_LOG(...) do { fprintf(stderr, "[ggml-hip] " __VA_ARGS__); fputc('\n', stderr); } while (0)

namespace {

struct hip_device_ctx { int id; std::string name, desc; ggml_backend_buffer_type buft; };
struct hip_backend_ctx {
    int device; bool kernel_error = false; void * stream = nullptr; void * wdata = nullptr; size_t wsize = 0; void * abuf = nullptr; size_t asize = 0; void * copy_event = nullptr;
    // replay of a token's launch list (graph_compute): the serialized arguments of every C-ABI call of the last graph, and the
    // captured graph of the list that came twice in a row
    std::vector<uint8_t> last_sig, graph_sig; void * graph_exec = nullptr; bool graph_broken = false; long replays = 0, captures = 0;
    // decode-ahead (see ahead_launch): the next step of a greedy decode started while the host is still busy with the current token
    struct scalar_set { const void * ptr; int32_t val; };
    struct {
        bool armed = false, inflight = false;
        bool chained = false;          // the step running ahead was queued BEHIND the step the host is still waiting for (ahead_launch(c, true)): synchronize() waits for `ev`, not for the stream
        bool tp = false;               // the step armed / running ahead is a tensor-parallel one (replayed through tp_ahead_replay, not graph_exec)
        bool ev_pending = false;       // ... and that event has not been waited for yet (EVERY synchronize() while the step runs ahead must stay off the stream: the host calls it more than once per token)
        bool snap_ready = false;       // the outputs' snapshot is complete although the step did not start (ahead_launch failed behind its argmax write): serve the pending read from it
        void * ev = nullptr, * table_dev = nullptr, * scratch = nullptr, * snap = nullptr; size_t snap_bytes = 0; int32_t * tok_host = nullptr;
        struct snap_rng { const void * src; void * dst; uint64_t bytes; }; void * rng_dev = nullptr; snap_rng * rng_host = nullptr; std::vector<snap_rng> rng_cur;      // the snapshot's ranges as the device holds them
        struct set_rec { const void * ptr; int32_t val, pad; }; set_rec * tab_host = nullptr;      // page-locked: the (pointer, absolute value) records of the step started ahead
        const void * ids_ptr = nullptr, * logits_ptr = nullptr; size_t logits_bytes = 0;
        struct out_range { const char * ptr; size_t bytes, snap_off; }; std::vector<out_range> outs;      // every OUTPUT tensor of the graph (snapshots)
        std::vector<scalar_set> last_sets, pred;
        int misses = 0; long graphs = 0, skip_until = 0, hits = 0, launched = 0;
    } ahead;
};
struct hip_buffer_ctx { int device; void * base; uint64_t uid; std::atomic<uint64_t> gen{0}; };     // gen: bumped by every write through the buffer interface
std::atomic<uint64_t> g_next_buffer_uid{1};     // (accessory models own their own contexts and may run on other threads)

// CLLM_HIP_STATS=1: where a token's wall time goes, seen from the module (host = everything between our entry points: the reference's
// graph build, scheduler split and allocation, sampling)
struct wall_stats {
    using clk = std::chrono::steady_clock;
    clk::time_point last_exit = clk::now();
    double host_us = 0, plan_us = 0, issue_us = 0, sync_us = 0, set_us = 0, get_us = 0, alloc_us = 0; long graphs = 0, calls = 0, sets = 0, gets = 0, allocs = 0, syncs = 0;
    static double us(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
} g_ws;
// every CLLM_HIP_* switch (csrc/options.def has their meaning): read ONCE through the library's table by ggml_backend_init, before the devices are registered;
// everything after that reads plain fields
struct host_options {
    bool stats = false, trace = false, sig_debug = false, tp_debug = false, ahead_debug = false, ahead_timing = false, ahead_sync = false, ahead_late = false;
    bool sync_load = false, force_stage = false, no_fuse = false, no_prefill_fuse = false, no_moe_down_fuse = false;
    bool pack = true, graph = true, moe_fold = true, ahead = true, ahead_chain = true, ahead_one = true, tp_streams = false, tp_head = true, tp_graph = true;
    int fuse_attn = 2, virtual_devices = 0, tp = 0;
    double pack_gb = -1.0;
    void read() {
        stats = cllm_option_is_set("CLLM_HIP_STATS"); trace = cllm_option_is_set("CLLM_HIP_TRACE"); sig_debug = cllm_option_is_set("CLLM_HIP_SIG_DEBUG");
        tp_debug = cllm_option_is_set("CLLM_HIP_TP_DEBUG"); ahead_debug = cllm_option_is_set("CLLM_HIP_AHEAD_DEBUG"); ahead_timing = cllm_option_is_set("CLLM_HIP_AHEAD_TIMING");
        ahead_sync = cllm_option_is_set("CLLM_HIP_AHEAD_SYNC"); ahead_late = cllm_option_is_set("CLLM_HIP_AHEAD_LATE"); sync_load = cllm_option_is_set("CLLM_HIP_SYNC_LOAD");
        force_stage = cllm_option_is_set("CLLM_HIP_FORCE_STAGE"); no_fuse = cllm_option_is_set("CLLM_HIP_NO_FUSE"); no_prefill_fuse = cllm_option_is_set("CLLM_HIP_NO_PREFILL_FUSE");
        no_moe_down_fuse = cllm_option_is_set("CLLM_HIP_NO_MOE_DOWN_FUSE");
        pack = cllm_option_int("CLLM_HIP_PACK") != 0; graph = cllm_option_int("CLLM_HIP_GRAPH") != 0; moe_fold = cllm_option_int("CLLM_HIP_MOE_FOLD") != 0;
        ahead = cllm_option_int("CLLM_HIP_AHEAD") != 0; ahead_chain = cllm_option_int("CLLM_HIP_AHEAD_CHAIN") != 0; ahead_one = cllm_option_int("CLLM_HIP_AHEAD_ONE") != 0;
        tp_streams = cllm_option_int("CLLM_HIP_TP_STREAMS") != 0; tp_head = cllm_option_int("CLLM_HIP_TP_HEAD") != 0; tp_graph = cllm_option_int("CLLM_HIP_TP_GRAPH") != 0;
        fuse_attn = cllm_option_int("CLLM_HIP_FUSE_ATTN"); virtual_devices = cllm_option_int("CLLM_HIP_VIRTUAL_DEVICES"); tp = cllm_option_int("CLLM_HIP_TP");
        pack_gb = cllm_option_real("CLLM_HIP_PACK_GB");
    }
} g_opt;
struct ws_scope {        // time inside one of our entry points goes to `slot`, the time since the previous one to host_us
    double & slot; wall_stats::clk::time_point t0;
    explicit ws_scope(double & s) : slot(s), t0(wall_stats::clk::now()) { if (g_opt.stats) g_ws.host_us += wall_stats::us(g_ws.last_exit, t0); }
    ~ws_scope() { if (g_opt.stats) { const auto t1 = wall_stats::clk::now(); slot += wall_stats::us(t0, t1); g_ws.last_exit = t1; } }
};

std::atomic<uint64_t> g_tp_kv_epoch{1};          // tensor parallel (tp_graph_compute): bumped by everything that may have changed the host's KV caches behind the ranks' shards
std::vector<hip_device_ctx *> g_devices;
ggml_backend_reg g_reg;

cllm_tensor desc(const ggml_tensor * t) {
    cllm_tensor d;
    d.type = (int32_t) t->type;
    for (int i = 0; i < 4; i++) { d.ne[i] = t->ne[i]; d.nb[i] = t->nb[i]; }
    d.data = t->data;
    return d;
}
size_t al256(size_t b) { return (b + 255) & ~(size_t) 255; }
// t seen as a dense F32 vector of K elements / as a dense F32 matrix of ne1 rows of ne0 elements
cllm_tensor as_vec(cllm_tensor t, int64_t K) { t.ne[0] = K; t.ne[1] = t.ne[2] = t.ne[3] = 1; t.nb[1] = t.nb[2] = t.nb[3] = (size_t) K * 4; return t; }
cllm_tensor as_mat(cllm_tensor t, int64_t ne0, int64_t ne1) { t.ne[0] = ne0; t.ne[1] = ne1; t.ne[2] = t.ne[3] = 1; t.nb[1] = (size_t) ne0 * 4; t.nb[2] = t.nb[3] = t.nb[1] * (size_t) ne1; return t; }
// the tuned and the coverage types (csrc/types.def: ggml_type and the cllm id are the same number, as desc() relies on); the coverage types take mat-mul and GET_ROWS
// only (gemv_kq.hip): no fused launch takes them
bool is_q(ggml_type t) { return is_quant_type((int) t); }
bool is_kq(ggml_type t) { return is_kq_type((int) t); }
bool dense_rows(const ggml_tensor * t) { return t->nb[0] == ggml_type_size(t->type); }
bool f32_dense(const ggml_tensor * t) { return t && t->type == GGML_TYPE_F32 && t->nb[0] == 4; }

// ---------------------------------------------------------------------------------------------------------------------------
// buffer
// ---------------------------------------------------------------------------------------------------------------------------
// Small set_tensor calls (chatllm writes the position vector of EVERY layer and the token id before each graph: 33 four-byte writes
// per token for Llama-3-8B, 14 us each as a synchronous copy) go through a page-locked ring: the caller's bytes are consumed when
// buf_set returns, the H2D copies are queued on the device's null stream and waited for ONCE, by whoever touches device memory next
// (graph_compute, get_tensor, cpy_tensor, synchronize, free_buffer).
// What the host last wrote into 4-byte tensors (position vectors, token id), by device address: chatllm gives every layer its own
// position tensor, all holding the same value -- knowing that, graph_compute builds the RoPE cos/sin table once per graph instead of
// once per layer (32 launches of 5 us per token for Llama-3-8B).  Any other write into the range forgets the entry.
std::unordered_map<const void *, int32_t> g_i32_vals;
// the 4-byte I32 tensors the host wrote since the last graph_compute, per device, in order (token id + one position per layer for chatllm):
// what decode-ahead predicts for the next step and checks its prediction against
std::vector<hip_backend_ctx::scalar_set> g_scalar_sets[64];
hip_backend_ctx * g_ahead_ctx[64] = {};          // the backend whose captured step may be running ahead on that device
// a write through the buffer interface that is not one of those scalars must not race a step running ahead (it may target memory that step uses)
void ahead_finish_event(hip_backend_ctx * c);
void ahead_quiesce(int device) {
    hip_backend_ctx * c = device >= 0 && device < 64 ? g_ahead_ctx[device] : nullptr;
    if (c && c->ahead.inflight) { ahead_finish_event(c); cllm_set_device(c->device); cllm_stream_sync(c->stream); }
}
void i32_forget(const void * lo, size_t n) {          // caller holds g_ring.m
    if (g_i32_vals.empty()) return;
    const char * a = (const char *) lo, * b = a + n;
    for (auto it = g_i32_vals.begin(); it != g_i32_vals.end();) { const char * k = (const char *) it->first; if (k + 4 > a && k < b) it = g_i32_vals.erase(it); else ++it; }
}
// Two page-locked rings share the scheme: `small` for the per-token scalars above, `bulk` for the loader -- chatllm uploads a model in 1,024,000-byte
// slices (TensorInfo::read_tensor_data, src/chat.cpp:1322-1338): a blocking copy + synchronize per slice leaves the DMA engine idle while the host
// reads the next slice from the file.  Through the bulk ring the slice is copied into pinned memory (its bytes are consumed when buf_set returns,
// as the interface requires), the H2D copy is queued and the host goes on reading; the ring is waited for only when it wraps (every 64 MiB).
struct set_ring {
    size_t cap, max; char * base = nullptr; size_t head = 0; bool failed = false; bool pending[64] = {}; std::mutex m;
    set_ring(size_t cap_, size_t max_) : cap(cap_), max(max_) {}
};
set_ring g_ring(256u << 10, 4096), g_bulk(64u << 20, 8u << 20);
void flush_ring(set_ring & r) {
    std::lock_guard<std::mutex> lock(r.m);
    for (int d = 0; d < 64; d++) if (r.pending[d]) {
        cllm_set_device(d);
        if (cllm_stream_sync(nullptr) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] queued set_tensor copies on device %d failed: %s\n", d, cllm_last_error());
        r.pending[d] = false;
    }
}
void flush_sets() { flush_ring(g_ring); flush_ring(g_bulk); }
bool ring_set(set_ring & r, int device, void * dst, const void * data, size_t size) {      // device already current
    std::lock_guard<std::mutex> lock(r.m);
    if (!r.base && !r.failed) { void * p = nullptr; if (cllm_host_malloc(&p, r.cap) == CLLM_OK) r.base = (char *) p; else r.failed = true; }
    if (!r.base || device < 0 || device >= 64 || size > r.max) return false;
    const size_t slot = (size + 63) & ~(size_t) 63;
    if (r.head + slot > r.cap) {            // wrap: every queued copy must have read its slot
        for (int d = 0; d < 64; d++) if (r.pending[d]) { cllm_set_device(d); cllm_stream_sync(nullptr); r.pending[d] = false; }
        cllm_set_device(device);
        r.head = 0;
    }
    memcpy(r.base + r.head, data, size);
    if (cllm_memcpy_h2d(dst, r.base + r.head, size, nullptr) != CLLM_OK) return false;
    r.head += slot; r.pending[device] = true;
    return true;
}
// a host buffer of any size into device memory: through the bulk ring (asynchronous), else a blocking copy
bool upload(int device, void * dst, const void * data, size_t size) {
    if (!g_opt.sync_load && ring_set(g_bulk, device, dst, data, size)) return true;
    return cllm_memcpy_h2d(dst, data, size, nullptr) == CLLM_OK && cllm_stream_sync(nullptr) == CLLM_OK;
}

void packs_forget(uint64_t uid);
void buf_free(ggml_backend_buffer_t b) {
    ws_scope ws(g_ws.alloc_us); g_ws.allocs++;
    flush_sets();
    auto * c = (hip_buffer_ctx *) b->context;
    ahead_quiesce(c->device);                      // a step running ahead may still use this memory
    if (c->device >= 0 && c->device < 64 && g_ahead_ctx[c->device]) g_ahead_ctx[c->device]->ahead.armed = false;
    { std::lock_guard<std::mutex> lock(g_ring.m); i32_forget(c->base, b->size); }
    cllm_set_device(c->device); packs_forget(c->uid); cllm_free(c->base); delete c;
}
void * buf_base(ggml_backend_buffer_t b) { return ((hip_buffer_ctx *) b->context)->base; }
void buf_memset(ggml_backend_buffer_t b, ggml_tensor * t, uint8_t v, size_t off, size_t size) {
    ahead_quiesce(((hip_buffer_ctx *) b->context)->device);
    cllm_set_device(((hip_buffer_ctx *) b->context)->device); ((hip_buffer_ctx *) b->context)->gen++; g_tp_kv_epoch++;
    { std::lock_guard<std::mutex> lock(g_ring.m); i32_forget((char *) t->data + off, size); }
    if (cllm_memset((char *) t->data + off, v, size, nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] memset_tensor '%s' failed: %s\n", t->name, cllm_last_error());
}
void buf_set(ggml_backend_buffer_t b, ggml_tensor * t, const void * data, size_t off, size_t size) {
    ws_scope ws(g_ws.set_us); g_ws.sets++;
    // called with 1,024,000-byte slices at arbitrary offsets while a model loads (src/chat.cpp:1322-1338): layout stays native
    auto * c = (hip_buffer_ctx *) b->context;
    cllm_set_device(c->device); c->gen++;
    bool scalar = true;
    {
        std::lock_guard<std::mutex> lock(g_ring.m);
        i32_forget((char *) t->data + off, size);
        if (size == 4 && off == 0 && t->type == GGML_TYPE_I32 && g_i32_vals.size() < 4096) memcpy(&g_i32_vals[t->data], data, 4);
        if (size == 4 && off == 0 && t->type == GGML_TYPE_I32 && c->device < 64) {
            hip_backend_ctx::scalar_set ss; ss.ptr = t->data; memcpy(&ss.val, data, 4);
            if (g_scalar_sets[c->device].size() < 1024) g_scalar_sets[c->device].push_back(ss);
            else scalar = false;                          // not recorded: must not be held back either (written through below, after the step running ahead has finished)
        } else scalar = false;
    }
    if (!scalar) { ahead_quiesce(c->device); g_tp_kv_epoch++; }
    // While a step runs ahead the device already holds the scalars that step needs, and ggml-alloc may have handed their memory to later nodes of the
    // same graph (the token id's block becomes part of the logits): a write now would land in the middle of -- or after -- the run and clobber it.
    // The value is recorded above; graph_compute either finds it equal to the prediction (nothing to write) or writes all of them before the real run.
    else if (c->device < 64 && g_ahead_ctx[c->device] && g_ahead_ctx[c->device]->ahead.inflight) return;
    if (size <= g_ring.max && ring_set(g_ring, c->device, (char *) t->data + off, data, size)) return;
    if (!upload(c->device, (char *) t->data + off, data, size)) GGML_LOG_ERROR("[ggml-hip] set_tensor '%s' (%zu bytes at %zu) failed: %s\n", t->name, size, off, cllm_last_error());
}
// get_tensor (the logits of every token: 513 KB for Llama-3): through a page-locked staging area -- the D2H copy into the host's pageable
// destination is several times slower than DMA into pinned memory + a memcpy
int tp_ahead_replay(hip_backend_ctx * c);
void * g_stage = nullptr; size_t g_stage_size = 0;
constexpr size_t k_stage_chunk = 4u << 20;
std::mutex g_stage_mutex;
void ahead_launch(hip_backend_ctx * c, bool chained = false);
void buf_get_impl(ggml_backend_buffer_t b, const char * src, const char * name, void * data, size_t size);
void buf_get(ggml_backend_buffer_t b, const ggml_tensor * t, void * data, size_t off, size_t size) {
    ws_scope ws(g_ws.get_us); g_ws.gets++;
    flush_sets();
    const int device = ((hip_buffer_ctx *) b->context)->device;
    hip_backend_ctx * ac = device >= 0 && device < 64 ? g_ahead_ctx[device] : nullptr;
    const char * src = (const char *) t->data + off;
    // the host reads the logits: the next step is started FIRST (it snapshots the graph's outputs on its stream, then runs), and the 513 KB copy to the host below is
    // served from that snapshot while the step already computes -- started after the copy, the GPU idled for the copy's ~70 us of every token
    const bool is_logits_read = ac && ac->ahead.armed && !ac->ahead.inflight && (const void *) t->data == ac->ahead.logits_ptr && off == 0 && size == ac->ahead.logits_bytes;
    if (is_logits_read && !g_opt.ahead_late) ahead_launch(ac);      // (CLLM_HIP_AHEAD_LATE, A/B: round 3's order)
    if (ac && (ac->ahead.inflight || (is_logits_read && ac->ahead.snap_ready))) {
        bool served = false;
        if (ac->ahead.inflight) ahead_finish_event(ac);      // (a host that reads without synchronize(): the snapshot must be complete)
        for (const auto & o : ac->ahead.outs)      // the step running ahead overwrites the graph's outputs: their snapshots
            if (src >= o.ptr && src + size <= o.ptr + o.bytes) { src = (const char *) ac->ahead.snap + o.snap_off + (src - o.ptr); served = true; break; }
        if (!served && ac->ahead.inflight) ahead_quiesce(device);        // anything else: what the step running ahead leaves behind
        ac->ahead.snap_ready = false;
    }
    buf_get_impl(b, src, t->name, data, size);
    if (is_logits_read && g_opt.ahead_late && ac->ahead.armed && !ac->ahead.inflight) ahead_launch(ac);
}
void buf_get_impl(ggml_backend_buffer_t b, const char * src, const char * name, void * data, size_t size) {
    std::lock_guard<std::mutex> lock(g_stage_mutex);            // one staging area (accessory models may read from other threads)
    cllm_set_device(((hip_buffer_ctx *) b->context)->device);
    const size_t want = size < k_stage_chunk ? size : k_stage_chunk;
    if (size >= 4096 && g_stage_size < want) {
        if (g_stage) cllm_host_free(g_stage);
        g_stage = nullptr; g_stage_size = 0;
        if (cllm_host_malloc(&g_stage, k_stage_chunk) == CLLM_OK) g_stage_size = k_stage_chunk;
    }
    if (size < 4096 || !g_stage) {
        if (cllm_memcpy_d2h(data, src, size, nullptr) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] get_tensor '%s' failed: %s\n", name, cllm_last_error());
        return;
    }
    for (size_t done = 0; done < size; done += g_stage_size) {
        const size_t n = size - done < g_stage_size ? size - done : g_stage_size;
        if (cllm_memcpy_d2h(g_stage, src + done, n, nullptr) != CLLM_OK) {     // synchronous
            GGML_LOG_ERROR("[ggml-hip] get_tensor '%s' failed: %s\n", name, cllm_last_error());
            return;
        }
        memcpy((char *) data + done, g_stage, n);
    }
}
bool buf_cpy(ggml_backend_buffer_t b, const ggml_tensor * src, ggml_tensor * dst) {
    if (!ggml_is_contiguous(src) || !ggml_is_contiguous(dst) || ggml_nbytes(src) != ggml_nbytes(dst)) return false;
    flush_sets();
    ahead_quiesce(((hip_buffer_ctx *) b->context)->device);
    if (src->buffer && src->buffer->iface.get_base == buf_base) ahead_quiesce(((hip_buffer_ctx *) src->buffer->context)->device);
    cllm_set_device(((hip_buffer_ctx *) b->context)->device); ((hip_buffer_ctx *) b->context)->gen++; g_tp_kv_epoch++;
    { std::lock_guard<std::mutex> lock(g_ring.m); i32_forget(dst->data, ggml_nbytes(dst)); }
    if (ggml_backend_buffer_is_host(src->buffer)) {
        if (cllm_memcpy_h2d(dst->data, src->data, ggml_nbytes(src), nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) { GGML_LOG_ERROR("[ggml-hip] cpy_tensor (host -> '%s') failed: %s\n", dst->name, cllm_last_error()); return false; }
        return true;
    }
    if (src->buffer && src->buffer->iface.get_base == buf_base) {     // another buffer of this module (any device: peer access through hipMemcpy)
        if (cllm_memcpy_d2d(dst->data, src->data, ggml_nbytes(src), nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) { GGML_LOG_ERROR("[ggml-hip] cpy_tensor ('%s' -> '%s') failed: %s\n", src->name, dst->name, cllm_last_error()); return false; }
        return true;
    }
    return false;
}
void buf_clear(ggml_backend_buffer_t b, uint8_t v) {
    auto * c = (hip_buffer_ctx *) b->context; ahead_quiesce(c->device); cllm_set_device(c->device); c->gen++; g_tp_kv_epoch++;
    { std::lock_guard<std::mutex> lock(g_ring.m); i32_forget(c->base, b->size); }
    if (cllm_memset(c->base, v, b->size, nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] clear failed: %s\n", cllm_last_error());
}
const ggml_backend_buffer_i k_buffer_i = { buf_free, buf_base, nullptr, buf_memset, buf_set, buf_get, buf_cpy, buf_clear, nullptr };

// ---------------------------------------------------------------------------------------------------------------------------
// packed weights: mat-vecs that read the same activation become ONE launch over a row-repacked copy of their weight matrices
//   q | k | v concatenated (the three projections of an attention block), gate / up with alternating rows (SiLU(gate)*up in the epilogue).
// The copy is made on the device the first time the pattern is seen (cllm_pack_rows) and stays valid as long as none of the source
// buffers is written through the buffer interface (generation counters) or freed.  It costs HBM -- the originals belong to the host and
// stay -- so the total is capped: CLLM_HIP_PACK_GB (default: a quarter of the device), and a tenth of the device must stay free.
// CLLM_HIP_PACK=0 turns it off.
// ---------------------------------------------------------------------------------------------------------------------------
struct pack_entry { void * data = nullptr; size_t bytes = 0; int n = 0; int device = 0; const void * src[3] = {}; uint64_t uid[3] = {}, gen[3] = {}; bool refused = false; };
std::unordered_map<const void *, pack_entry> g_packs;          // keyed by the first source's data pointer
size_t g_pack_bytes = 0;
std::mutex g_pack_mutex;                                        // (accessory models own their own contexts and may run on other threads)
void packs_forget(uint64_t uid) {
    std::lock_guard<std::mutex> lock(g_pack_mutex);
    for (auto it = g_packs.begin(); it != g_packs.end();) {
        bool hit = false;
        for (int i = 0; i < it->second.n; i++) hit = hit || it->second.uid[i] == uid;
        if (hit) { if (it->second.data) { cllm_free(it->second.data); g_pack_bytes -= it->second.bytes; } it = g_packs.erase(it); } else ++it;
    }
}
bool ours(const ggml_tensor * t) { return t && t->buffer && t->buffer->iface.free_buffer == buf_free && !t->view_src; }
// the packed copy of n (2 or 3) same-type, same-row-length weight matrices, or nullptr (not ours / over budget / allocation failed)
void * get_pack(int device, void * stream, const ggml_tensor * const * w, int n, bool interleave, bool flat = false) {      // flat: byte blobs (bias vectors)
    if (!g_opt.pack) return nullptr;
    for (int i = 0; i < n; i++) if (!ours(w[i]) || ((const hip_buffer_ctx *) w[i]->buffer->context)->device != device) return nullptr;
    std::lock_guard<std::mutex> lock(g_pack_mutex);
    pack_entry & e = g_packs[w[0]->data];
    bool valid = e.n == n && e.device == device;
    for (int i = 0; i < n && valid; i++) {
        const auto * bc = (const hip_buffer_ctx *) w[i]->buffer->context;
        valid = e.src[i] == w[i]->data && e.uid[i] == bc->uid && e.gen[i] == bc->gen.load();
    }
    if (valid) return e.refused ? nullptr : e.data;
    if (e.data) { cllm_stream_sync(stream); cllm_free(e.data); g_pack_bytes -= e.bytes; }
    e = pack_entry(); e.n = n; e.device = device; e.refused = true;
    size_t bytes = 0; int64_t rows[3]; const void * srcs[3];
    for (int i = 0; i < n; i++) {
        const auto * bc = (const hip_buffer_ctx *) w[i]->buffer->context;
        e.src[i] = w[i]->data; e.uid[i] = bc->uid; e.gen[i] = bc->gen.load();
        if (!flat && w[i]->ne[2] > 1 && w[i]->nb[2] != (size_t) w[i]->ne[1] * w[i]->nb[1]) return nullptr;      // expert slabs must be contiguous
        rows[i] = flat ? (int64_t) ggml_nbytes(w[i]) : w[i]->ne[1] * w[i]->ne[2]; srcs[i] = w[i]->data; bytes += flat ? ggml_nbytes(w[i]) : (size_t) rows[i] * w[i]->nb[1];
    }
    size_t mfree = 0, mtotal = 0;
    cllm_device_info(device, nullptr, 0, &mfree, &mtotal, nullptr);
    const double cap_gb = g_opt.pack_gb;
    const size_t cap = cap_gb >= 0 ? (size_t)(cap_gb * 1e9) : mtotal / 4;
    if (g_pack_bytes + bytes > cap || mfree < bytes + mtotal / 10) return nullptr;
    void * p = nullptr;
    if (cllm_malloc(&p, bytes) != CLLM_OK) return nullptr;
    if (cllm_pack_rows(stream, p, srcs, rows, n, flat ? 1 : w[0]->nb[1], interleave ? 1 : 0) != CLLM_OK || cllm_stream_sync(stream) != CLLM_OK) { cllm_free(p); return nullptr; }
    e.data = p; e.bytes = bytes; e.refused = false; g_pack_bytes += bytes;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// buffer type
// ---------------------------------------------------------------------------------------------------------------------------
const char * buft_name(ggml_backend_buffer_type_t t) { return ((hip_device_ctx *) t->context)->name.c_str(); }
ggml_backend_buffer_t buft_alloc(ggml_backend_buffer_type_t t, size_t size) {
    ws_scope ws(g_ws.alloc_us); g_ws.allocs++;
    auto * d = (hip_device_ctx *) t->context;
    cllm_set_device(d->id);
    void * p = nullptr;
    if (cllm_malloc(&p, size ? size : 1) != CLLM_OK) { HIPB_LOG("alloc of %zu bytes failed: %s", size, cllm_last_error()); return nullptr; }
    return ggml_backend_buffer_init(t, k_buffer_i, new hip_buffer_ctx{ d->id, p, g_next_buffer_uid.fetch_add(1) }, size);
}
size_t buft_align(ggml_backend_buffer_type_t) { return 256; }
bool buft_is_host(ggml_backend_buffer_type_t) { return false; }
const ggml_backend_buffer_type_i k_buft_i = { buft_name, buft_alloc, buft_align, nullptr, nullptr, buft_is_host };

// ---------------------------------------------------------------------------------------------------------------------------
// supports_op: exactly the combinations cllm_op_* accept (anything else goes to the CPU backend through the scheduler)
// ---------------------------------------------------------------------------------------------------------------------------
bool dev_supports_op(ggml_backend_dev_t, const ggml_tensor * op) {
    const ggml_tensor * a = op->src[0], * b = op->src[1];
    switch (op->op) {
        case GGML_OP_NONE: case GGML_OP_RESHAPE: case GGML_OP_VIEW: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE: return true;
        case GGML_OP_MUL_MAT:
            // an F16 b with an F16 a (the IM2COL operand of ggml_conv_1d / _2d): check_mm's predicates for it -- dense halves, strides that are multiples of 2
            if (b && b->type == GGML_TYPE_F16)
                return a->type == GGML_TYPE_F16 && op->type == GGML_TYPE_F32 && dense_rows(a) && b->nb[0] == 2 && b->nb[1] % 2 == 0 && b->nb[2] % 2 == 0 && b->nb[3] % 2 == 0 &&
                       a->ne[2] * a->ne[3] <= 65535;
            if (!f32_dense(b) || op->type != GGML_TYPE_F32 || !dense_rows(a)) return false;
            // (the predicates of cllm_op_mul_mat / check_mm that do not depend on the data pointers: what is declined here runs on the CPU backend
            // instead of failing in graph_compute; buffers of this module are 256-byte aligned and ggml-alloc keeps that alignment)
            if (is_q(a->type)) return a->ne[0] % 32 == 0 && b->nb[1] % 16 == 0 && b->nb[2] % 16 == 0 && b->nb[3] % 16 == 0 &&
                                      (a->type != GGML_TYPE_Q4_K || (a->nb[1] % 16 == 0 && a->nb[2] % 16 == 0 && a->nb[3] % 16 == 0)) &&
                                      (a->type != GGML_TYPE_Q4_1 || (a->nb[1] % 4 == 0 && a->nb[2] % 4 == 0 && a->nb[3] % 4 == 0));
            if (is_kq(a->type)) return a->ne[0] % ggml_blck_size(a->type) == 0 && b->nb[1] % 16 == 0 && b->nb[2] % 16 == 0 && b->nb[3] % 16 == 0 && (a->type != GGML_TYPE_Q5_K || a->nb[1] % 16 == 0) &&
                                       (a->type == GGML_TYPE_MXFP4 || a->nb[1] % 2 == 0);
            return (a->type == GGML_TYPE_F16 || a->type == GGML_TYPE_F32) && a->ne[2] * a->ne[3] <= 65535;
        case GGML_OP_MUL_MAT_ID:
            if (is_kq(a->type))        // the coverage types: one grid slice per (token, slot) of gemv_kq.hip (no fused MoE launch takes them)
                return f32_dense(b) && op->src[2] && op->src[2]->type == GGML_TYPE_I32 && a->ne[3] == 1 && b->ne[3] == 1 && a->ne[0] % ggml_blck_size(a->type) == 0 && dense_rows(a) &&
                       (b->ne[1] == 1 || b->ne[1] == op->src[2]->ne[0]) && op->src[2]->ne[0] * op->src[2]->ne[1] <= 65535 && b->nb[1] % 16 == 0 && b->nb[2] % 16 == 0 &&
                       (a->type != GGML_TYPE_Q5_K || (a->nb[1] % 16 == 0 && a->nb[2] % 16 == 0)) && (a->type == GGML_TYPE_MXFP4 || (a->nb[1] % 2 == 0 && a->nb[2] % 2 == 0));
            return is_q(a->type) && f32_dense(b) && op->src[2] && op->src[2]->type == GGML_TYPE_I32 && a->ne[3] == 1 && b->ne[3] == 1 && a->ne[0] % 32 == 0 &&
                   (b->ne[1] == 1 || b->ne[1] == op->src[2]->ne[0]) && op->src[2]->ne[0] * op->src[2]->ne[1] <= 65535 && b->nb[1] % 16 == 0 && b->nb[2] % 16 == 0 &&
                   (a->type != GGML_TYPE_Q4_K || (a->nb[1] % 16 == 0 && a->nb[2] % 16 == 0)) && (a->type != GGML_TYPE_Q4_1 || (a->nb[1] % 4 == 0 && a->nb[2] % 4 == 0));
        case GGML_OP_RMS_NORM: return f32_dense(a) && op->type == GGML_TYPE_F32;
        case GGML_OP_NORM: {       // cllm_op_norm's own predicates: dense F32 rows on both sides, eps >= 0 (not NaN); MUL and ADD of a LayerNorm's affine stay their own nodes
            float eps; memcpy(&eps, op->op_params, 4);
            return f32_dense(a) && op->type == GGML_TYPE_F32 && op->nb[0] == 4 && eps >= 0.0f;
        }
        case GGML_OP_L2_NORM: {    // cllm_op_l2_norm's own predicates: dense F32 rows on both sides, eps >= 0 (not NaN)
            float eps; memcpy(&eps, op->op_params, 4);
            return f32_dense(a) && f32_dense(op) && eps >= 0.0f;
        }
        case GGML_OP_GROUP_NORM:   // cllm_op_group_norm's: dense F32 rows on both sides, n_groups > 0 (eps as it is); MUL and ADD of a GroupNorm's affine stay their own nodes
            return f32_dense(a) && f32_dense(op) && op->op_params[0] > 0 && a->ne[2] * a->ne[3] <= 0x7fffffff;
        case GGML_OP_ADD: case GGML_OP_MUL: case GGML_OP_DIV: return a->type == GGML_TYPE_F32 && b->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && ggml_can_repeat(b, a);
        case GGML_OP_SUM_ROWS: return f32_dense(a) && f32_dense(op);
        case GGML_OP_TOP_K: return f32_dense(a) && op->type == GGML_TYPE_I32 && a->ne[0] <= 4096;
        case GGML_OP_SCALE: case GGML_OP_DIAG_MASK_INF: return a->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32;
        case GGML_OP_UNARY: switch (ggml_get_unary_op(op)) {      // the codes of cllm_unary (ggml::act's nodes, src/layers.cpp:441-485)
            case GGML_UNARY_OP_SILU: case GGML_UNARY_OP_TANH: case GGML_UNARY_OP_RELU: case GGML_UNARY_OP_SIGMOID: case GGML_UNARY_OP_GELU: case GGML_UNARY_OP_GELU_QUICK:
                return f32_dense(a) && f32_dense(op);
            default: return false;
        }
        case GGML_OP_SQR: return f32_dense(a) && f32_dense(op);
        case GGML_OP_ROPE: {
            const int mode = op->op_params[2];
            return f32_dense(a) && f32_dense(op) && b && b->type == GGML_TYPE_I32 && (mode == 0 || mode == 2) && (!op->src[2] || op->src[2]->type == GGML_TYPE_F32);
        }
        case GGML_OP_SOFT_MAX: {
            float max_bias; memcpy(&max_bias, (const float *) op->op_params + 1, 4);
            return f32_dense(a) && f32_dense(op) && max_bias == 0.0f && !op->src[2] && (!b || b->type == GGML_TYPE_F32 || b->type == GGML_TYPE_F16);
        }
        case GGML_OP_SET_ROWS:
            if (op->type == GGML_TYPE_Q8_0) return f32_dense(a) && a->ne[0] % 32 == 0 && a->nb[1] % 16 == 0 && a->nb[2] % 16 == 0 && a->nb[3] % 16 == 0 && (b->type == GGML_TYPE_I32 || b->type == GGML_TYPE_I64);
            return f32_dense(a) && (op->type == GGML_TYPE_F16 || op->type == GGML_TYPE_F32) && (b->type == GGML_TYPE_I32 || b->type == GGML_TYPE_I64);
        case GGML_OP_FLASH_ATTN_EXT: {      // what cllm_op_flash_attn_ext takes (`-fa`, src/layers.cpp:2634-2656); anything else stays on the CPU backend
            const ggml_tensor * v = op->src[2], * m = op->src[3];
            float max_bias, softcap; memcpy(&max_bias, (const float *) op->op_params + 1, 4); memcpy(&softcap, (const float *) op->op_params + 2, 4);
            if (!a || !b || !v || op->src[4] || max_bias != 0.0f || softcap != 0.0f || op->type != GGML_TYPE_F32 || a->type != GGML_TYPE_F32 || a->nb[0] != 4) return false;
            if (b->type != v->type || (b->type != GGML_TYPE_F16 && b->type != GGML_TYPE_Q8_0) || b->nb[0] != ggml_type_size(b->type) || v->nb[0] != ggml_type_size(v->type)) return false;
            const int64_t D = a->ne[0];
            if ((D != 64 && D != 128) || b->ne[0] != D || v->ne[0] != D || v->ne[1] != b->ne[1] || b->ne[2] <= 0 || a->ne[2] % b->ne[2] || v->ne[2] != b->ne[2] || a->ne[3] != b->ne[3] || a->ne[3] != v->ne[3]) return false;
            if (a->nb[1] % 16 || a->nb[2] % 16 || a->nb[3] % 16 || !ggml_is_contiguous(op)) return false;
            if (b->type == GGML_TYPE_F16 && (b->nb[1] % 16 || b->nb[2] % 16 || b->nb[3] % 16 || v->nb[1] % 16 || v->nb[2] % 16 || v->nb[3] % 16)) return false;
            if (m && (m->type != GGML_TYPE_F16 || !ggml_is_contiguous(m) || m->ne[0] < b->ne[1] || m->ne[1] < a->ne[1])) return false;
            // the C ABI's own predicates (cllm_op_flash_attn_ext): a mask broadcasts over heads / batches only as 1 or the full count (ggml allows any divisor)
            if (m && ((m->ne[2] != 1 && m->ne[2] != a->ne[2]) || (m->ne[3] != 1 && m->ne[3] != a->ne[3]))) return false;
            // (q's data pointer must be 16-byte aligned as well: every block ggml-alloc hands out is aligned to the buffer type's 256 bytes and the reference's
            //  q is a PERMUTE of a contiguous projection -- checked again at run time, where a mismatch is an error rather than a fallback)
            return a->ne[2] <= 65535 && a->ne[3] <= 65535;
        }
        case GGML_OP_CPY: case GGML_OP_DUP: case GGML_OP_CONT: {
            const ggml_type s = a->type, d = op->type;
            const bool fs = s == GGML_TYPE_F32 || s == GGML_TYPE_F16, fd = d == GGML_TYPE_F32 || d == GGML_TYPE_F16;
            if (s == d && is_q(s)) return a->ne[0] == op->ne[0] && a->nb[0] == ggml_type_size(s) && op->nb[0] == ggml_type_size(s);      // whole quantized rows (CONT of the Q8_0 K-cache view)
            return (fs && fd) || (s == GGML_TYPE_I32 && d == GGML_TYPE_I32);
        }
        case GGML_OP_IM2COL: {     // cllm_op_im2col's own predicates (a: the kernel, read for its shape and type; b: the image); dst ne is ggml_im2col's by construction
            const int32_t * q = op->op_params;      // s0, s1, p0, p1, d0, d1, is_2D
            const bool two = q[6] == 1;
            if (q[6] != 0 && q[6] != 1) return false;
            if (!a || !f32_dense(b) || (op->type != GGML_TYPE_F16 && op->type != GGML_TYPE_F32) || (op->type == GGML_TYPE_F16 && a->type != GGML_TYPE_F16) || !ggml_is_contiguous(op)) return false;
            if (q[0] <= 0 || q[4] <= 0 || q[2] < 0 || q[3] < 0 || (two && (q[1] <= 0 || q[5] <= 0))) return false;
            if (two ? a->ne[2] != b->ne[2] : (a->ne[1] != b->ne[1] || b->ne[3] != 1)) return false;
            if (two && b->ne[1] > 1 && b->nb[1] != (size_t) b->ne[0] * 4) return false;
            const size_t ofs0 = two ? b->nb[3] : b->nb[2], ofs1 = two ? b->nb[2] : b->nb[1];
            return ofs0 <= 0x7fffffff && ofs1 <= 0x7fffffff && ofs0 % 4 == 0 && ofs1 % 4 == 0 && op->ne[0] <= 0x7fffffff;
        }
        case GGML_OP_POOL_1D: case GGML_OP_POOL_2D: {      // cllm_op_pool_1d / _2d's: F32 and contiguous on both sides, op MAX | AVG, k, s > 0, p >= 0 (dst ne is the constructor's)
            const int32_t * q = op->op_params;      // 1-D: op, k0, s0, p0; 2-D: op, k0, k1, s0, s1, p0, p1
            if (!a || a->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || !ggml_is_contiguous(a) || !ggml_is_contiguous(op) || (q[0] != GGML_OP_POOL_MAX && q[0] != GGML_OP_POOL_AVG)) return false;
            // the entries recompute dst ne from the int parameters (ggml_calc_pool_output_size, in float as there); ggml_pool_2d computes it from its float paddings and
            // stores them truncated, so a fractional padding may give another ne: such a node stays on the CPU backend
            auto out = [](int64_t ins, int ks, int s, int p) { return (int64_t)(((float) ins + 2.0f * (float) p - (float) ks) / (float) s + 1.0f); };
            if (op->op == GGML_OP_POOL_1D) return q[1] > 0 && q[2] > 0 && q[3] >= 0 && a->ne[0] + 2 * (int64_t) q[3] + q[1] <= 0x7fffffff && op->ne[0] == out(a->ne[0], q[1], q[2], q[3]);
            return q[1] > 0 && q[2] > 0 && q[3] > 0 && q[4] > 0 && q[5] >= 0 && q[6] >= 0 && (int64_t) q[1] * q[2] <= 0x7fffffff &&
                   a->ne[0] + 2 * (int64_t) q[5] + q[1] <= 0x7fffffff && a->ne[1] + 2 * (int64_t) q[6] + q[2] <= 0x7fffffff &&
                   op->ne[0] == out(a->ne[0], q[1], q[3], q[5]) && op->ne[1] == out(a->ne[1], q[2], q[4], q[6]);
        }
        // the four cases below restate cllm_op_pad / _pad_reflect_1d / _upscale / _conv_transpose_1d's own predicates, with two exceptions that hold for every tensor of a
        // graph: the entries' tests of the data pointers (every one of the four tests them for 4-byte or element alignment) are left out, because this module's buffers
        // are 256-byte aligned, ggml-alloc keeps that alignment and the host cuts its views at whole elements (a pointer that is off all the same fails the entry, and with it graph_compute); and cllm_op_upscale's ne >= 0 is left out,
        // because a ggml tensor has no negative ne.  dst ne is the constructor's
        case GGML_OP_PAD: {        // lp0, rp0, .., lp3, rp3, circular
            const int32_t * q = op->op_params;
            if (!a || a->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || !ggml_is_contiguous(op) || q[8] != 0) return false;
            for (int i = 0; i < 4; i++) if (q[2 * i] < 0 || q[2 * i + 1] < 0 || op->ne[i] != a->ne[i] + q[2 * i] + q[2 * i + 1] || a->nb[i] % 4) return false;
            return true;
        }
        case GGML_OP_PAD_REFLECT_1D: {
            const int32_t * q = op->op_params;      // p0, p1
            return a && a->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && ggml_is_contiguous(a) && ggml_is_contiguous(op) && q[0] >= 0 && q[1] >= 0 && q[0] < a->ne[0] && q[1] < a->ne[0] &&
                   op->ne[0] == a->ne[0] + q[0] + q[1] && op->ne[1] == a->ne[1] && op->ne[2] == a->ne[2] && op->ne[3] == a->ne[3];
        }
        case GGML_OP_UPSCALE: {    // op_params[0]: the mode and its flag bits; NEAREST and BILINEAR with no flag (what ggml::interpolate emits), align-corners, antialias and bicubic stay on the CPU
            const int32_t mode = op->op_params[0];
            if (!a || a->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || !ggml_is_contiguous(op) || (mode != GGML_SCALE_MODE_NEAREST && mode != GGML_SCALE_MODE_BILINEAR)) return false;
            return a->nb[0] % 4 == 0 && a->nb[1] % 4 == 0 && a->nb[2] % 4 == 0 && a->nb[3] % 4 == 0 && (ggml_nelements(op) == 0 || ggml_nelements(a) != 0);
        }
        case GGML_OP_CONV_TRANSPOSE_1D: {      // a: the kernel [K, Cout, Cin], b: the data [L, Cin]; op_params: s0, p0, d0
            const int32_t * q = op->op_params;
            if (!a || !b || (a->type != GGML_TYPE_F16 && a->type != GGML_TYPE_F32) || !f32_dense(b) || op->type != GGML_TYPE_F32 || !dense_rows(a) || !ggml_is_contiguous(op)) return false;
            if (q[0] <= 0 || q[1] != 0 || q[2] != 1) return false;
            const size_t es = ggml_type_size(a->type);
            return a->ne[3] == 1 && b->ne[2] == 1 && b->ne[3] == 1 && b->ne[1] == a->ne[2] && op->ne[0] == (b->ne[0] - 1) * q[0] + a->ne[0] && op->ne[1] == a->ne[1] && op->ne[2] == 1 && op->ne[3] == 1 &&
                   a->nb[1] % es == 0 && a->nb[2] % es == 0 && b->nb[1] % 4 == 0;
        }
        case GGML_OP_GET_ROWS: return (is_q(a->type) || is_kq(a->type) || a->type == GGML_TYPE_F16 || a->type == GGML_TYPE_F32) && b->type == GGML_TYPE_I32 && op->type == GGML_TYPE_F32;
        default: return false;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backend (stream): graph_compute
// ---------------------------------------------------------------------------------------------------------------------------
int ensure_wdata(hip_backend_ctx * c, size_t need) {
    if (need <= c->wsize) return CLLM_OK;
    cllm_stream_sync(c->stream);                    // kernels in flight may still read the old scratch
    if (c->wdata) cllm_free(c->wdata);
    c->wdata = nullptr; c->wsize = 0;
    const size_t sz = need + need / 4 + 4096;
    if (int rc = cllm_malloc(&c->wdata, sz)) return rc;
    c->wsize = sz;
    return CLLM_OK;
}

int ensure_abuf(hip_backend_ctx * c, size_t need) {      // fused attention: cos/sin table | q,k,v projections | long-context scores
    if (need <= c->asize) return CLLM_OK;
    cllm_stream_sync(c->stream);
    if (c->abuf) cllm_free(c->abuf);
    c->abuf = nullptr; c->asize = 0;
    const size_t sz = need + need / 4 + 4096;
    if (int rc = cllm_malloc(&c->abuf, sz)) return rc;
    c->asize = sz;
    return CLLM_OK;
}

#include "fuse_plan.h"          // the fusion planner: fuse_plan, make_plan

// ---- launch-list replay ---------------------------------------------------------------------------------------------------
// The reference rebuilds, re-splits and re-allocates its graph for every token (src/models.cpp:1244-1312), but for a decode step the
// result is the same list of C-ABI calls with the same arguments as the token before: everything that changes (token id, position)
// is read from device memory by the kernels, and ggml's allocator hands out the same addresses.  graph_compute therefore walks the
// nodes twice: first only serializing every call's arguments; if the bytes equal those of a captured graph, that graph is launched
// (one host call, no per-launch gaps on the GPU) instead of the ~160 launches; if they equal the previous token's list, this token's
// launches are captured on the way.  Any difference -- another address, shape, scalar, fusion decision -- simply issues the calls.
// Measured (Llama-3-8B Q4_K through the unmodified host, one MI355X): the host time inside graph_compute drops from 586 to 74 us per
// token, but the token is GPU-bound -- issue + synchronize is 1.75 ms either way (the launches were already running ahead of the GPU) --
// so wall time barely moves -- but the host thread is free ~0.5 ms earlier per token and the GPU sees no launch gaps.  ON by default
// (CLLM_HIP_GRAPH=0 turns it off); every replayed list is byte-identical to the calls it stands for (tests/test_gpu_dropin.py).
struct sig_writer {
    std::vector<uint8_t> & b;
    void raw(const void * p, size_t n) { const uint8_t * q = (const uint8_t *) p; b.insert(b.end(), q, q + n); }
    template <class T> void put(const T & v) { static_assert(std::is_trivially_copyable<T>::value, "pod"); raw(&v, sizeof(v)); }
    void arg(const cllm_tensor * t) { if (!t) { put((uint8_t) 0); return; } put((uint8_t) 1); put(t->type); raw(t->ne, sizeof(t->ne)); raw(t->nb, sizeof(t->nb)); put(t->data); }
    void arg(cllm_tensor * t) { arg((const cllm_tensor *) t); }
    void arg(const cllm_rope_params * r) { if (r) put(*r); else put((uint8_t) 0); }
    void arg(cllm_rope_params * r) { arg((const cllm_rope_params *) r); }
    void arg(std::nullptr_t) { put((uint8_t) 0); }
    template <class T> typename std::enable_if<std::is_arithmetic<T>::value || std::is_pointer<T>::value || std::is_enum<T>::value>::type arg(T v) { put(v); }
    std::vector<size_t> * marks = nullptr;        // (CLLM_HIP_SIG_DEBUG: where every call starts)
    template <class... A> void call(const void * fn, A... a) { if (marks) marks->push_back(b.size()); put(fn); int dummy[] = { 0, (arg(a), 0)... }; (void) dummy; }
};

// ---- decode-ahead.  chatllm's host is synchronous: compute, synchronize, read the logits, sample, build the next graph (~0.5 ms for Llama-3-8B),
//      compute ...  -- the GPU idles while the host works.  In the steady state of a greedy decode the next step is known before the host asks for it:
//      same captured launch list, token = argmax(logits), every position + 1.  So right after the host has read the logits the module starts that step
//      itself (argmax + scalar updates on the device, then the captured graph); when the host's graph_compute arrives, its launch list and the scalars
//      it wrote are compared with the prediction: equal -> the work is already running (or done), nothing is launched; different -> the step runs again
//      the normal way (what ran ahead only touched the logits, scratch and the cache row of the next position, all of which the real step rewrites).
//      Guards: only after a replayed step; only if the logits are the graph's single output; positions stay inside the caches; any other access through
//      the buffer interface waits for the step running ahead (ahead_quiesce) and the logits stay readable from a snapshot; two misses in a row switch
//      it off for the next 64 graphs (a sampling host costs itself at most a few % that way).  CLLM_HIP_AHEAD=0 turns it off.
// chained (round 6): called from graph_compute itself, right behind the launch of the step the host asked for -- the snapshot of that step's outputs, the arg-max and the next
// step are queued on the stream before the host has even synchronized; synchronize() then waits for `ev` (outputs snapshotted, next token known) instead of the whole stream, and
// the GPU goes from one step into the next without waiting for the host to wake up, read and come back (~80 us per token: 682 vs 722 tok/s through the host in round 5).
// Still at most ONE step runs ahead of what the host has asked for.
void ahead_finish_event(hip_backend_ctx * c) {       // the chained step's event has not been waited for yet: wait, and bring the host-side mirror of the scalars in step
    auto & A = c->ahead;
    if (!A.ev_pending) return;
    A.ev_pending = false;
    cllm_set_device(c->device);
    cllm_event_sync(A.ev);
    std::lock_guard<std::mutex> lock(g_ring.m);
    for (const auto & ss : A.pred) { const int32_t v = ss.ptr == A.ids_ptr ? A.tok_host[0] : ss.val; auto it = g_i32_vals.find(ss.ptr); if (it != g_i32_vals.end()) it->second = v; }
}
void ahead_launch(hip_backend_ctx * c, bool chained) {
    auto & A = c->ahead;
    A.armed = false; A.snap_ready = false; A.chained = false; A.ev_pending = false;
    cllm_set_device(c->device);
    if (!A.ev && cllm_event_create(&A.ev) != CLLM_OK) return;
    if (!A.tok_host) { void * p = nullptr; if (cllm_host_malloc(&p, 64) != CLLM_OK) return; A.tok_host = (int32_t *) p; }
    if (!A.table_dev && cllm_malloc(&A.table_dev, 1024 * 16) != CLLM_OK) return;
    if (!A.tab_host) { void * p = nullptr; if (cllm_host_malloc(&p, 1024 * 16) != CLLM_OK) return; A.tab_host = (decltype(A.tab_host)) p; }
    if (!A.scratch) { if (cllm_malloc(&A.scratch, 4096) != CLLM_OK) return; if (cllm_memset(A.scratch, 0, 4096, nullptr) != CLLM_OK || cllm_stream_sync(nullptr) != CLLM_OK) return; }
    if (!A.rng_dev && cllm_malloc(&A.rng_dev, 16 * 24) != CLLM_OK) return;
    if (!A.rng_host) { void * p = nullptr; if (cllm_host_malloc(&p, 16 * 24) != CLLM_OK) return; A.rng_host = (decltype(A.rng_host)) p; }
    size_t snap_need = 0;
    for (auto & o : A.outs) { o.snap_off = snap_need; snap_need += al256(o.bytes); }
    if (A.snap_bytes < snap_need) {
        if (A.snap) { cllm_stream_sync(c->stream); cllm_free(A.snap); A.snap = nullptr; A.snap_bytes = 0; A.rng_cur.clear(); }
        if (cllm_malloc(&A.snap, snap_need) != CLLM_OK) return;
        A.snap_bytes = snap_need;
    }
    // the scalars of the next step as ABSOLUTE values (the position scalars + 1; the token id comes from the argmax): the device words are not read -- ggml-alloc may
    // have handed their blocks to later nodes of the graph that just ran.  One record per distinct pointer (the host's last write of a step wins).
    A.pred.clear();
    int n_rec = 0;
    for (const auto & ss : A.last_sets) {
        A.pred.push_back(ss);
        if (ss.ptr == A.ids_ptr) continue;
        A.pred.back().val = ss.val + 1;
        int k = 0; while (k < n_rec && A.tab_host[k].ptr != ss.ptr) k++;
        if (k == n_rec) { if (n_rec >= 1024) return; n_rec++; }
        A.tab_host[k].ptr = ss.ptr; A.tab_host[k].val = ss.val + 1; A.tab_host[k].pad = 0;
    }
    void * st = c->stream;
    // CLLM_HIP_AHEAD_TIMING=1 (diagnosis): per step, on the GPU's clock -- the captured step alone, what stands in front of it (table copy, prep launch, event), and the token
    // period; a ring of four event triples, read two launches later (the host has synchronized on a later event by then, also with the chain on)
    static void * t_p[4] = {}, * t_g0[4] = {}, * t_g1[4] = {}; static long t_n = 0; static double acc_graph = 0, acc_prep = 0, acc_period = 0; static long acc_n = 0;
    const bool timing = g_opt.ahead_timing;
    const int t_k = (int)(t_n & 3);
    if (timing) {
        if (!t_p[0]) for (int i = 0; i < 4; i++) { cllm_event_create(&t_p[i]); cllm_event_create(&t_g0[i]); cllm_event_create(&t_g1[i]); }
        if (t_n >= 3) {
            const int a = (int)((t_n - 3) & 3), b = (int)((t_n - 2) & 3);
            float g = 0, q = 0, per = 0;
            if (cllm_event_elapsed_ms(t_g0[a], t_g1[a], &g) == CLLM_OK && cllm_event_elapsed_ms(t_p[a], t_g0[a], &q) == CLLM_OK && cllm_event_elapsed_ms(t_g0[a], t_g0[b], &per) == CLLM_OK) { acc_graph += g; acc_prep += q; acc_period += per; acc_n++; }
            if (acc_n == 64) { HIPB_LOG("ahead timing over 64 steps (GPU clock): token period %.1f us = captured step %.1f + table copy / prep launch / event in front of it %.1f + idle %.1f", acc_period / 64 * 1e3, acc_graph / 64 * 1e3, acc_prep / 64 * 1e3, (acc_period - acc_graph - acc_prep) / 64 * 1e3); acc_graph = acc_prep = acc_period = 0; acc_n = 0; }
        }
        cllm_event_record(t_p[t_k], st);
    }
    if (n_rec && cllm_memcpy_h2d(A.table_dev, A.tab_host, (size_t) n_rec * 16, st) != CLLM_OK) return;      // queued on the step's stream from page-locked memory; done before the event below
    // the snapshot of the outputs, the arg-max and the scalar updates: ONE launch (cllm_op_snapshot_argmax_set; CLLM_HIP_AHEAD_ONE=0: round 5's copies + two launches)
    bool fused_prep = g_opt.ahead_one && A.outs.size() <= 16;
    for (const auto & o : A.outs) fused_prep = fused_prep && o.bytes % 4 == 0;
    if (fused_prep) {
        bool same = A.rng_cur.size() == A.outs.size();
        for (size_t k = 0; same && k < A.outs.size(); k++) same = A.rng_cur[k].src == (const void *) A.outs[k].ptr && A.rng_cur[k].dst == (void *)((char *) A.snap + A.outs[k].snap_off) && A.rng_cur[k].bytes == A.outs[k].bytes;
        if (!same) {                               // (the ranges move only when ggml-alloc moves the outputs: the table is uploaded once per captured graph)
            cllm_stream_sync(st);                  // a queued launch may still read the table
            A.rng_cur.clear();
            for (size_t k = 0; k < A.outs.size(); k++) { A.rng_cur.push_back({ (const void *) A.outs[k].ptr, (void *)((char *) A.snap + A.outs[k].snap_off), (uint64_t) A.outs[k].bytes }); A.rng_host[k] = A.rng_cur.back(); }
            if (cllm_memcpy_h2d(A.rng_dev, A.rng_host, A.outs.size() * 24, st) != CLLM_OK) { A.rng_cur.clear(); return; }
        }
    } else for (const auto & o : A.outs) if (cllm_memcpy_d2d((char *) A.snap + o.snap_off, o.ptr, o.bytes, st) != CLLM_OK) { cllm_stream_sync(st); return; }
    // From here on the arg-max below may already have written the token id -- into a block ggml-alloc may have made part of the logits.  If anything fails now the
    // step does not run ahead, but the host's pending read must still see the logits as they were: the snapshot (complete once the stream is idle) serves it.
    auto fail_behind_the_snapshot = [&]() { if (cllm_stream_sync(st) == CLLM_OK) A.snap_ready = true; };
    if (fused_prep) {
        if (cllm_op_snapshot_argmax_set(st, A.rng_dev, (int) A.outs.size(), (const float *) A.logits_ptr, (int64_t)(A.logits_bytes / 4), (int32_t *) A.ids_ptr, A.tok_host, A.table_dev, n_rec, A.scratch) != CLLM_OK) { cllm_stream_sync(st); return; }
    } else
    if (cllm_op_argmax_set(st, (const float *) A.logits_ptr, (int64_t)(A.logits_bytes / 4), (int32_t *) A.ids_ptr, A.tok_host, A.table_dev, n_rec, A.scratch) != CLLM_OK) { fail_behind_the_snapshot(); return; }
    if (cllm_event_record(A.ev, st) != CLLM_OK) { fail_behind_the_snapshot(); return; }
    if (timing) cllm_event_record(t_g0[t_k], st);
    if ((A.tp ? tp_ahead_replay(c) : cllm_graph_launch(c->graph_exec, st)) != CLLM_OK) { fail_behind_the_snapshot(); return; }
    if (timing) { cllm_event_record(t_g1[t_k], st); t_n++; }
    if (g_opt.ahead_sync) cllm_stream_sync(st);       // (debugging: run the step ahead to completion before returning)
    A.inflight = true; A.launched++; A.chained = chained; A.ev_pending = true;
    // not chained: the snapshot and the scalars are in place before the host goes on (its own writes of the same scalars come later); the device then holds the predicted
    // scalars: the host-side mirror is brought in step (the host will write the same values again).  Chained: synchronize() does both.
    if (!chained) ahead_finish_event(c);
}


// a step is running ahead: is it the one the host is asking for?  1: yes (nothing to launch), 0: no -- the step was allowed to finish and the host's scalars are in place (buf_set
// held them back), -1: error.  sig_equal: the host's launch list equals the captured one the step was started with.
int ahead_resolve(hip_backend_ctx * c, bool sig_equal, const std::vector<hip_backend_ctx::scalar_set> & cur_sets) {
    auto & A = c->ahead;
    ahead_finish_event(c);                 // (a host that did not synchronize since: the predicted token must be known before the comparison below)
    A.inflight = false;
    bool ok = sig_equal && cur_sets.size() == A.pred.size();
    for (size_t k = 0; ok && k < cur_sets.size(); k++)
        ok = cur_sets[k].ptr == A.pred[k].ptr && cur_sets[k].val == (A.pred[k].ptr == A.ids_ptr ? A.tok_host[0] : A.pred[k].val);
    if (ok) { A.hits++; A.misses = 0; return 1; }
    if (g_opt.ahead_debug) {
        HIPB_LOG("ahead: MISS sig_equal=%d sets %zu predicted %zu", (int) sig_equal, cur_sets.size(), A.pred.size());
        for (size_t k = 0; k < cur_sets.size() && k < A.pred.size(); k++) {
            const int32_t want = A.pred[k].ptr == A.ids_ptr ? A.tok_host[0] : A.pred[k].val;
            if (cur_sets[k].ptr != A.pred[k].ptr || cur_sets[k].val != want)
                HIPB_LOG("ahead:   set %zu: host wrote %p = %d, predicted %p = %d%s", k, cur_sets[k].ptr, (int) cur_sets[k].val, A.pred[k].ptr, (int) want, A.pred[k].ptr == A.ids_ptr ? " (token id)" : "");
        }
    }
    if (++A.misses >= 2) { A.skip_until = A.graphs + 64; A.misses = 0; }
    cllm_set_device(c->device);
    cllm_stream_sync(c->stream);           // the step that ran ahead is not the one asked for: let it finish (every rank's stream joins this one), then put the host's scalars in place
    for (const auto & ss : cur_sets) if (cllm_memcpy_h2d((void *) ss.ptr, &ss.val, 4, nullptr) != CLLM_OK) { HIPB_LOG("scalar write failed: %s", cllm_last_error()); return -1; }
    if (cllm_stream_sync(nullptr) != CLLM_OK) return -1;
    return 0;
}

#include "tp_step.h"            // tensor parallel behind the boundary: g_tp, tp_graph_compute, tp_ahead_replay

// arm decode-ahead for the token after this one (see ahead_launch) -- and, with the chain on, start that step right away.  have_graph: this step was replayed from a captured
// launch list (one graph, or the tensor-parallel device's graph per stream) that the next step can be started with.
void ahead_arm(hip_backend_ctx * c, ggml_cgraph * g, const fuse_plan & plan, const std::vector<hip_backend_ctx::scalar_set> & cur_sets, bool have_graph, bool tp) {
    const bool ahead_off = !g_opt.ahead;
    auto & A = c->ahead;
    A.armed = false;
    const int nn = ggml_graph_n_nodes(g);
    if (ahead_off || !have_graph || A.graphs < A.skip_until || cur_sets.empty() || nn <= 0 || plan.attns.empty() || c->device >= 64) return;
    const ggml_tensor * out = ggml_graph_node(g, nn - 1), * ids = nullptr;
    int n_out = 0; A.outs.clear(); bool ok = out->type == GGML_TYPE_F32 && ggml_is_contiguous(out) && out->data && ggml_nbytes(out) % 4 == 0 && ggml_nbytes(out) >= 8;
    int64_t min_ml = INT64_MAX;
    for (const fused_attn & F : plan.attns) { ok = ok && F.level == 2; if (F.ML < min_ml) min_ml = F.ML; }
    for (int i = 0; ok && i < nn; i++) {
        const ggml_tensor * t = ggml_graph_node(g, i);
        if (t->flags & GGML_TENSOR_FLAG_OUTPUT) { n_out++; if (t->data && ggml_is_contiguous(t)) A.outs.push_back({ (const char *) t->data, ggml_nbytes(t), 0 }); else ok = false; }
        if (!plan.skip[i] && (t->op == GGML_OP_SET_ROWS || t->op == GGML_OP_FLASH_ATTN_EXT)) ok = false;      // cache writes outside the fused block, growing masks: not predicted (experts are picked on the device: nothing to predict)
        if (!ids && t->op == GGML_OP_GET_ROWS && t->src[1] && t->src[1]->type == GGML_TYPE_I32 && ggml_nelements(t->src[1]) == 1) ids = t->src[1];
    }
    if (!(out->flags & GGML_TENSOR_FLAG_OUTPUT)) A.outs.push_back({ (const char *) out->data, ggml_nbytes(out), 0 });
    ok = ok && ids && ids->data && n_out <= 8;
    bool has_ids = false;
    for (const auto & ss : cur_sets) { if (ids && ss.ptr == ids->data) has_ids = true; else if ((int64_t) ss.val + 1 >= min_ml || ss.val < 0) ok = false; }
    if (g_opt.ahead_debug) HIPB_LOG("ahead: ok=%d has_ids=%d ids=%p n_out=%d out_flag=%d min_ml=%lld sets=%zu out=%s(%s) bytes=%zu", (int) ok, (int) has_ids, ids ? ids->data : nullptr, n_out, (int)((out->flags & GGML_TENSOR_FLAG_OUTPUT) != 0), (long long) min_ml, cur_sets.size(), out->name, ggml_op_name(out->op), ggml_nbytes(out));
    if (!ok || !has_ids) return;
    A.ids_ptr = ids->data; A.logits_ptr = out->data; A.logits_bytes = ggml_nbytes(out); A.last_sets = cur_sets;
    A.armed = true; A.tp = tp; g_ahead_ctx[c->device] = c;
    // the next step goes out NOW, behind the one just launched (CLLM_HIP_AHEAD_CHAIN=0: when the host reads the logits, round 5's order)
    if (g_opt.ahead_chain) ahead_launch(c, true);
}

const char * be_name(ggml_backend_t b) { return ((hip_device_ctx *) b->device->context)->name.c_str(); }      // (the ggml device's name: several of them can sit on one GPU, CLLM_HIP_VIRTUAL_DEVICES)
void be_free(ggml_backend_t b) {
    auto * c = (hip_backend_ctx *) b->context;
    cllm_set_device(c->device); cllm_stream_sync(c->stream);
    if (c->wdata) cllm_free(c->wdata);
    if (c->abuf) cllm_free(c->abuf);
    if (c->graph_exec) cllm_graph_destroy(c->graph_exec);
    if (c->copy_event) cllm_event_destroy(c->copy_event);
    if (c->device < 64 && g_ahead_ctx[c->device] == c) g_ahead_ctx[c->device] = nullptr;
    if (g_tp.owner == c) { tp_free_all(); cllm_set_device(c->device); }      // (tensor parallel: the ranks' streams, shards and receive buffers hang off this backend's stream)
    if (c->ahead.ev) cllm_event_destroy(c->ahead.ev);
    if (c->ahead.tok_host) cllm_host_free(c->ahead.tok_host);
    if (c->ahead.table_dev) cllm_free(c->ahead.table_dev);
    if (c->ahead.tab_host) cllm_host_free(c->ahead.tab_host);
    if (c->ahead.scratch) cllm_free(c->ahead.scratch);
    if (c->ahead.rng_dev) cllm_free(c->ahead.rng_dev);
    if (c->ahead.rng_host) cllm_host_free(c->ahead.rng_host);
    if (c->ahead.snap) cllm_free(c->ahead.snap);
    cllm_stream_destroy(c->stream);
    delete c; delete b;
}
void be_sync(ggml_backend_t b) {
    ws_scope ws(g_ws.sync_us); g_ws.syncs++;
    flush_sets();
    auto * c = (hip_backend_ctx *) b->context; cllm_set_device(c->device);
    // a step queued behind the one the host waits for (ahead_launch chained): the host's step is complete -- outputs snapshotted -- when the event behind its arg-max has fired
    if (c->ahead.inflight && c->ahead.chained) ahead_finish_event(c); else cllm_stream_sync(c->stream);
    cllm_stream_sync(nullptr);
    // a bounded wait inside a kernel that timed out leaves void results behind: synchronize() cannot return a status (ggml-backend-impl.h:96), so it is said
    // loudly here and the next graph_compute of this backend fails
    if (cllm_check_kernel_errors() != CLLM_OK) { GGML_LOG_ERROR("[ggml-hip] %s\n", cllm_last_error()); c->kernel_error = true; }
    if (!tp_check_errors()) { GGML_LOG_ERROR("[ggml-hip] tensor parallel: a granule wait of the fused all-reduce timed out (a rank is late, dead or out of step): the step's logits are void\n"); c->kernel_error = true; }
}

// ---- single device: the steps of be_graph_compute -------------------------------------------------------------------------
void trace_graph(ggml_cgraph * g) {
    HIPB_LOG("graph_compute: %d nodes", ggml_graph_n_nodes(g));
    for (int i = 0; i < ggml_graph_n_nodes(g); i++) {
        const ggml_tensor * n = ggml_graph_node(g, i);
        fprintf(stderr, "  %3d %-14s %-24s [%lld,%lld,%lld,%lld] nb0=%zu", i, ggml_op_name(n->op), n->name, (long long) n->ne[0], (long long) n->ne[1], (long long) n->ne[2], (long long) n->ne[3], n->nb[0]);
        for (int k = 0; k < 3; k++) if (n->src[k]) fprintf(stderr, "  s%d=%s(%s)[%lld,%lld,%lld]", k, n->src[k]->name, ggml_op_name(n->src[k]->op), (long long) n->src[k]->ne[0], (long long) n->src[k]->ne[1], (long long) n->src[k]->ne[2]);
        fputc('\n', stderr);
    }
}
void trace_plan(ggml_cgraph * g, const fuse_plan & plan) {
    for (const fused_mv & f : plan.mvs) if (f.node >= 0) fprintf(stderr, "  plan: mat-vec node %d pro %d%s%s%s\n", f.node, f.pro, f.resid ? " +resid" : "", f.alias ? " STAGED (dst overlaps an input)" : "", f.group >= 0 ? " grouped" : "");
    for (const fused_attn & A : plan.attns) fprintf(stderr, "  plan: attention level %d%s\n", A.level, A.alias ? " STAGED" : "");
    for (int i = 0; i < ggml_graph_n_nodes(g); i++) if (!plan.skip[i]) { const ggml_tensor * n = ggml_graph_node(g, i); if (n->op == GGML_OP_ADD || n->op == GGML_OP_MUL || n->op == GGML_OP_CPY || n->op == GGML_OP_CONT) fprintf(stderr, "  plan: node %d %s launched on its own (alt %d)\n", i, ggml_op_name(n->op), plan.alt[i]); }
}

// another backend context of this device (a draft / embedding / accessory model) has a step running ahead: buf_set held this graph's scalar writes back
// for THAT context's hit test -- they are ours.  Let the step finish, put them in place, and leave that context to run its next step the normal way.
bool settle_foreign_ahead(hip_backend_ctx * c, const std::vector<hip_backend_ctx::scalar_set> & cur_sets) {
    if (!(c->device < 64 && g_ahead_ctx[c->device] && g_ahead_ctx[c->device] != c && g_ahead_ctx[c->device]->ahead.inflight)) return true;
    hip_backend_ctx * o = g_ahead_ctx[c->device];
    ahead_quiesce(c->device);
    o->ahead.inflight = false; o->ahead.armed = false; o->ahead.misses = 0;
    cllm_set_device(c->device);
    for (const auto & ss : cur_sets) if (cllm_memcpy_h2d((void *) ss.ptr, &ss.val, 4, nullptr) != CLLM_OK) { HIPB_LOG("scalar write failed: %s", cllm_last_error()); return false; }
    return cllm_stream_sync(nullptr) == CLLM_OK;
}

// scratch of the fused forms: [cos/sin table 1 KB][q | k | v projections][SiLU(gate)*up activation][scores of the long-context attention][staged outputs]
struct fusion_scratch {
    size_t qkv_bytes = 0, act_bytes = 0, score_bytes = 0, stage_bytes = 0;
    float * cs = nullptr, * qkv = nullptr, * act = nullptr, * stage = nullptr; void * scores = nullptr;
    bool needed() const { return qkv_bytes || act_bytes || stage_bytes; }
    size_t total() const { return 1024 + qkv_bytes + act_bytes + score_bytes + stage_bytes; }
};
fusion_scratch fusion_scratch_sizes(ggml_cgraph * g, const fuse_plan & plan) {
    fusion_scratch S;
    auto grow = [](size_t & slot, size_t b) { if (b > slot) slot = b; };
    for (const fused_attn & A : plan.attns) if (A.level == 2) { grow(S.qkv_bytes, al256((size_t) A.hd * (A.nh + 2 * A.nkv) * 4)); grow(S.score_bytes, cllm_attn_decode_wsize(A.n_kv, A.nh, A.ML)); }
    for (const merge_group & G : plan.groups) if (G.interleave) grow(S.act_bytes, al256((size_t) ggml_graph_node(g, plan.mvs[G.member[0]].node)->ne[0] * 4));
    // staged: outputs of fused launches whose dst aliases one of their inputs (see make_plan)
    for (const fused_mv & f : plan.mvs) if (f.alias) grow(S.stage_bytes, al256((size_t) ggml_graph_node(g, f.node)->src[0]->ne[1] * 4));
    for (const fused_attn & A : plan.attns) if (A.alias) grow(S.stage_bytes, al256((size_t) A.nh * A.hd * 4));
    for (const fused_fa & F : plan.fas) if (F.alias) grow(S.stage_bytes, al256(F.bytes));
    return S;
}
void fusion_scratch_bind(fusion_scratch & S, void * abuf) {      // abuf holds S.total() bytes (ensure_abuf)
    char * b = (char *) abuf;
    S.cs = (float *) b; b += 1024; S.qkv = (float *) b; b += S.qkv_bytes; S.act = (float *) b; b += S.act_bytes; S.scores = b; b += S.score_bytes; S.stage = (float *) b;
}
// level 2: the q / k / v mat-vecs write into module scratch, where the attention launch reads them
void patch_qkv_dst(fuse_plan & plan, const fusion_scratch & S) {
    for (const fused_attn & A : plan.attns) if (A.level == 2) {
        plan.mvs[A.wq].dst = S.qkv; plan.mvs[A.wk].dst = S.qkv + (size_t) A.hd * A.nh; plan.mvs[A.wv].dst = S.qkv + (size_t) A.hd * (A.nh + A.nkv);
    }
}

// merged expert gate/up launches: only where a packed (per-expert interleaved) copy of the two weight tensors can be had (planning that needs get_pack, hence here)
void resolve_moe_gate_up(hip_backend_ctx * c, ggml_cgraph * g, fuse_plan & plan) {
    for (moe_gate_up & G : plan.gus) {
        const ggml_tensor * w[2] = { ggml_graph_node(g, G.gate)->src[0], ggml_graph_node(g, G.up)->src[0] };
        G.W = get_pack(c->device, c->stream, w, 2, true);
        if (!G.W) continue;
        plan.skip[G.gate] = plan.skip[G.up] = 1;            // (the UNARY is skipped already)
        plan.alt[G.mul] = ALT_MOE_GATE_UP; plan.moe[G.mul] = (int)(&G - plan.gus.data());
        // the block's router into the same launch (one launch less per sparse-MoE block): the experts read the ids of a router launch whose normalised activation feeds nothing but
        // that router and these two MUL_MAT_IDs, router and experts share one weight type, and whatever else reads the probabilities / ids runs after this node (or is itself fused away)
        const bool fold = g_opt.moe_fold;
        const ggml_tensor * gm = ggml_graph_node(g, G.gate);
        for (size_t ri = 0; fold && ri < plan.routers.size(); ri++) {
            moe_router & R = plan.routers[ri];
            if (R.itk < 0 || plan.skip[R.itk] || plan.alt[R.itk] != ALT_MOE_ROUTER || ggml_graph_node(g, R.itk) != gm->src[2] || R.gate->type != gm->src[0]->type) continue;
            const ggml_tensor * act = gm->src[1];
            while (act != R.xnorm && (act->op == GGML_OP_RESHAPE || act->op == GGML_OP_VIEW) && act->src[0] && act->src[0]->data == act->data) act = act->src[0];
            if (act != R.xnorm || ggml_nelements(gm->src[1]) != R.xnorm->ne[0]) continue;
            bool ok = R.xn_users.size() == 2 && ((R.xn_users[0] == G.gate && R.xn_users[1] == G.up) || (R.xn_users[0] == G.up && R.xn_users[1] == G.gate));
            for (int u : R.out_users) if (u != G.gate && u != G.up && !plan.skip[u] && u <= G.mul) ok = false;
            // the fold moves the router from the TOP_K node to the later MUL node: the launch there still READS R.x, and its fallback (two launches) WRITES R.xnorm -- blocks
            // ggml-alloc may have handed to a node in between (their last readers precede the MUL).  Nothing launched in (TOP_K, MUL] may overlap either.
            for (int j = R.itk + 1; ok && j <= G.mul; j++) {
                const ggml_tensor * t = ggml_graph_node(g, j);
                if (plan.skip[j] || !t->data || t->op == GGML_OP_NONE || t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_PERMUTE || t->op == GGML_OP_TRANSPOSE) continue;
                const size_t kb = (size_t) R.xnorm->ne[0] * 4;
                if (overlap(t->data, ggml_nbytes(t), R.x->data, kb) || overlap(t->data, ggml_nbytes(t), R.xnorm->data, kb)) ok = false;
            }
            if (!ok) continue;
            G.router = (int) ri; plan.skip[R.itk] = 1;
            break;
        }
    }
}

// ---- the walk over the nodes: ONE code path both issues and serializes.  With a sig_writer every C-ABI call's arguments go into the launch list instead of
//      to the device (same decisions, same host-side state changes) ----
struct emitter {
    sig_writer * sw = nullptr;
    template <class F, class... A> int operator()(F fn, A... a) const { if (sw) { sw->call((const void *) fn, a...); return CLLM_OK; } return fn(a...); }
};
struct walk_ctx {
    hip_backend_ctx * c; ggml_cgraph * g; void * st; const fusion_scratch & S; emitter call;
    int merged = 0, launches = 0;
    const int32_t * tab_pos = nullptr; int tab_hd = 0; float tab_fb = 0.0f;      // what S.cs holds (computed once per graph, not per layer)
};
struct node_io { ggml_tensor * n; const ggml_tensor * a, * b; cllm_tensor d, da, db; };      // a node, its first two sources and their descriptors

int issue_flash_prefill(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const fused_fa & F = plan.fas[plan.moe[i]];
    const ggml_tensor * kq = ggml_graph_node(w.g, F.ikq);
    cllm_tensor dk = desc(kq->src[0]), dq = desc(kq->src[1]);
    if (!F.alias) return w.call(cllm_op_attn_prefill, w.st, &dq, &dk, &io.da, &io.d, F.scale, F.n_past);
    cllm_tensor ds = io.d; ds.data = w.S.stage;
    int rc = w.call(cllm_op_attn_prefill, w.st, &dq, &dk, &io.da, &ds, F.scale, F.n_past);
    if (rc == CLLM_OK) rc = w.call(cllm_memcpy_d2d, (void *) io.n->data, (const void *) w.S.stage, F.bytes, w.st);
    return rc;
}
// a fused mat-vec: the first member of a group in node order launches for all of them -- if a packed copy of the weights can be had
int issue_fused_mat_vec(walk_ctx & w, fuse_plan & plan, int i, node_io & io) {
    const fused_mv & f = plan.mvs[plan.mv[i]];
    void * st = w.st; float * a_act = w.S.act, * a_stage = w.S.stage;
    int rc = CLLM_OK;
    if (f.group >= 0) {
        merge_group & G = plan.groups[f.group];
        if (G.state == 0) {
            const ggml_tensor * wt[3]; int64_t rows = 0;
            for (int k = 0; k < G.n; k++) { wt[k] = ggml_graph_node(w.g, plan.mvs[G.member[k]].node)->src[0]; rows += wt[k]->ne[1]; }
            void * W = get_pack(w.c->device, st, wt, G.n, G.interleave);
            const float * Bv = nullptr;
            if (W && G.bias) {
                const ggml_tensor * bt[3];
                for (int k = 0; k < G.n; k++) bt[k] = plan.mvs[G.member[k]].resid_t;
                Bv = (const float *) get_pack(w.c->device, st, bt, G.n, false, true);
                if (!Bv) W = nullptr;
            }
            G.state = 2;
            if (W) {
                cllm_tensor dw = desc(wt[0]); dw.ne[1] = rows; dw.nb[2] = dw.nb[3] = (size_t) rows * dw.nb[1]; dw.data = W;
                rc = w.call(cllm_op_mul_mat_vec_fused, st, &dw, 1, f.px, f.pw, f.eps, G.interleave ? 1 : 0, Bv, G.interleave ? a_act : plan.mvs[G.member[0]].dst);
                if (rc == CLLM_OK) {
                    G.state = 1; w.merged++;
                    if (G.consumer >= 0) { fused_mv & d = plan.mvs[G.consumer]; d.pro = 2; d.px = a_act; d.pw = nullptr; }
                } else if (rc == CLLM_E_UNSUPPORTED) rc = CLLM_OK;      // shape the merged form does not take: launch the members
            }
        }
        if (G.state == 1 || rc != CLLM_OK) return rc;
    }
    if (!f.alias) return w.call(cllm_op_mul_mat_vec_fused, st, &io.da, f.pro, f.px, f.pw, f.eps, 0, f.resid, f.dst);
    // staged: dst overlaps px / pw (with an in-place residual the staged launch still reads resid == the final dst: no hazard)
    rc = w.call(cllm_op_mul_mat_vec_fused, st, &io.da, f.pro, f.px, f.pw, f.eps, 0, f.resid, a_stage);
    if (rc == CLLM_OK) rc = w.call(cllm_memcpy_d2d, (void *) f.dst, (const void *) a_stage, (size_t) io.a->ne[1] * 4, st);
    return rc;
}
int issue_prefill_mat_mul(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const pf_mm & F = plan.pfs[plan.pf[i]];
    hip_backend_ctx * c = w.c; cllm_tensor & da = io.da, & db = io.db;
    if (int rc = ensure_wdata(c, cllm_mul_mat_wsize(&da, &db))) return rc;
    cllm_tensor dx = F.pro == 5 ? db : desc(F.x), dw2, dr, dout = F.out ? desc(F.out) : io.d;
    if (F.pro == 1) dx = as_mat(dx, db.ne[0], db.ne[1]);
    if (F.w2) { dw2 = desc(F.w2); if (F.pro == 1) dw2 = as_vec(dw2, db.ne[0]); }
    if (F.resid) dr = desc(F.resid);
    return w.call(cllm_op_mul_mat_ex, w.st, &da, &dx, &dout, c->wdata, c->wsize, F.pro, F.w2 ? &dw2 : nullptr, F.eps, 0, F.resid ? &dr : nullptr);
}
int issue_mat_mul(walk_ctx & w, node_io & io) {
    hip_backend_ctx * c = w.c;
    if (int rc = ensure_wdata(c, cllm_mul_mat_wsize(&io.da, &io.db))) return rc;
    return w.call(cllm_op_mul_mat, w.st, &io.da, &io.db, &io.d, c->wdata, c->wsize);
}
int issue_mat_mul_id(walk_ctx & w, node_io & io) {
    hip_backend_ctx * c = w.c;
    cllm_tensor dc = desc(io.n->src[2]);
    if (int rc = ensure_wdata(c, cllm_mul_mat_wsize(&io.da, &io.db))) return rc;
    return w.call(cllm_op_mul_mat_id, w.st, &io.da, &io.db, &dc, &io.d, c->wdata, c->wsize);
}
int issue_moe_combine(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const fused_moe & M = plan.moes[plan.moe[i]];
    const int64_t H = M.experts->ne[0], T = M.experts->ne[2];
    cllm_tensor de = desc(M.experts), dp = as_mat(desc(M.probs), M.probs->ne[0], T), di = desc(M.ids), dr, dd = as_mat(io.d, H, T);
    if (M.resid) dr = as_mat(desc(M.resid), H, T);
    if (M.down < 0) return w.call(cllm_op_moe_combine, w.st, &de, &dp, &di, M.resid ? &dr : nullptr, &dd);
    const ggml_tensor * mm = ggml_graph_node(w.g, M.down);
    cllm_tensor dw = desc(mm->src[0]), dx = desc(mm->src[1]);
    return w.call(cllm_op_mul_mat_id_combine, w.st, &dw, &dx, &di, &dp, M.resid ? &dr : nullptr, &dd);
}
int issue_moe_gate_up(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const moe_gate_up & G = plan.gus[plan.moe[i]];
    const ggml_tensor * gm = ggml_graph_node(w.g, G.gate);
    cllm_tensor dw = desc(gm->src[0]), dx = desc(gm->src[1]), di = desc(gm->src[2]);
    dw.ne[1] *= 2; dw.nb[2] *= 2; dw.nb[3] = dw.nb[2] * (size_t) dw.ne[2]; dw.data = G.W;
    if (G.router < 0) return w.call(cllm_op_mul_mat_id_silu_mul, w.st, &dw, &dx, &di, &io.d);
    const moe_router & R = plan.routers[G.router];
    const int64_t K = R.xnorm->ne[0];
    cllm_tensor rx = as_vec(desc(R.x), K), rw = as_vec(desc(R.w), K), rg = desc(R.gate), rn = as_vec(desc(R.xnorm), K), rp = desc(R.probs), rt = desc(ggml_graph_node(w.g, R.itk));
    int rc = w.call(cllm_op_moe_router_gate_up, w.st, &rx, &rw, R.eps, &rg, &dw, &rp, &rt, &io.d);
    if (rc == CLLM_E_UNSUPPORTED) {              // the two launches it replaces
        rc = w.call(cllm_op_moe_router, w.st, &rx, &rw, R.eps, &rg, &rn, &rp, &rt);
        if (rc == CLLM_OK) rc = w.call(cllm_op_mul_mat_id_silu_mul, w.st, &dw, &dx, &di, &io.d);
    }
    return rc;
}
int issue_mul(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    if (plan.alt[i] == ALT_MOE_GATE_UP) return issue_moe_gate_up(w, plan, i, io);
    if (plan.alt[i] == ALT_SILU_MUL || plan.alt[i] == ALT_MUL_SILU) {
        const bool a_is_silu = plan.alt[i] == ALT_SILU_MUL;
        const ggml_tensor * gate = (a_is_silu ? io.a : io.b)->src[0], * up = a_is_silu ? io.b : io.a;
        cllm_tensor dg = desc(gate), du = desc(up);
        return w.call(cllm_op_silu_mul, w.st, &dg, &du, &io.d);
    }
    if (plan.alt[i] == ALT_RMS_NORM_MUL) {
        float eps; memcpy(&eps, io.a->op_params, 4);
        cllm_tensor dx = desc(io.a->src[0]), dwt = as_vec(desc(io.b), io.n->ne[0]);
        return w.call(cllm_op_rms_norm_mul, w.st, &dx, &dwt, &io.d, eps);
    }
    return w.call(cllm_op_mul, w.st, &io.da, &io.db, &io.d);
}
int issue_moe_router(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const moe_router & R = plan.routers[plan.moe[i]];
    const int64_t K = R.xnorm->ne[0];
    cllm_tensor dx = as_vec(desc(R.x), K), dwt = as_vec(desc(R.w), K), dg = desc(R.gate), dn = as_vec(desc(R.xnorm), K), dp = desc(R.probs);
    return w.call(cllm_op_moe_router, w.st, &dx, &dwt, R.eps, &dg, &dn, &dp, &io.d);
}
int issue_rope(walk_ctx & w, node_io & io) {
    const ggml_tensor * n = io.n;
    cllm_rope_params p;
    p.n_dims = n->op_params[1]; p.mode = n->op_params[2]; p.n_ctx_orig = n->op_params[4];
    memcpy(&p.freq_base, n->op_params + 5, 4); memcpy(&p.freq_scale, n->op_params + 6, 4); memcpy(&p.ext_factor, n->op_params + 7, 4);
    memcpy(&p.attn_factor, n->op_params + 8, 4); memcpy(&p.beta_fast, n->op_params + 9, 4); memcpy(&p.beta_slow, n->op_params + 10, 4);
    cllm_tensor dc;
    if (n->src[2]) dc = desc(n->src[2]);
    return w.call(cllm_op_rope, w.st, &io.da, &io.db, n->src[2] ? &dc : nullptr, &io.d, &p);
}
int issue_soft_max(walk_ctx & w, const fuse_plan & plan, int i, node_io & io) {
    const ggml_tensor * n = io.n;
    if (plan.sm_src[i] >= 0) {
        const ggml_tensor * sc = ggml_graph_node(w.g, plan.sm_src[i]);
        float scale; memcpy(&scale, sc->op_params, 4);
        cllm_tensor ds = desc(sc->src[0]);
        return w.call(cllm_op_scale_mask_soft_max, w.st, &ds, &io.d, scale, n->src[0]->op_params[0]);
    }
    float scale, max_bias; memcpy(&scale, n->op_params, 4); memcpy(&max_bias, (const float *) n->op_params + 1, 4);
    return w.call(cllm_op_soft_max, w.st, &io.da, io.b ? &io.db : nullptr, &io.d, scale, max_bias);
}
int issue_flash_attn_ext(walk_ctx & w, node_io & io) {
    const ggml_tensor * n = io.n; hip_backend_ctx * c = w.c;
    float scale, max_bias, softcap; memcpy(&scale, n->op_params, 4); memcpy(&max_bias, (const float *) n->op_params + 1, 4); memcpy(&softcap, (const float *) n->op_params + 2, 4);
    cllm_tensor dc = desc(n->src[2]), dm;
    if (n->src[3]) dm = desc(n->src[3]);
    if (int rc = ensure_wdata(c, cllm_flash_attn_wsize(&io.da))) return rc;
    return w.call(cllm_op_flash_attn_ext, w.st, &io.da, &io.db, &dc, n->src[3] ? &dm : nullptr, &io.d, scale, max_bias, softcap, c->wdata, c->wsize);
}
// the single-token attention block in place of its CONT node (level 2: with RoPE and the cache writes; level 1: the last seven nodes)
int issue_attention(walk_ctx & w, const fuse_plan & plan, int i) {
    const fused_attn & A = plan.attns[plan.attn[i]];
    const fusion_scratch & S = w.S; void * st = w.st;
    if (A.level == 2) {
        const bool table = A.hd == 64 || A.hd == 128;       // head sizes of the compact kernels
        bool have = w.tab_hd == A.hd && w.tab_fb == A.freq_base && w.tab_pos != nullptr;
        if (have && w.tab_pos != A.pos) {                   // another layer's position tensor: the same value, as far as the host's writes tell?
            std::lock_guard<std::mutex> lock(g_ring.m);
            const auto x = g_i32_vals.find(w.tab_pos), y = g_i32_vals.find(A.pos);
            have = x != g_i32_vals.end() && y != g_i32_vals.end() && x->second == y->second;
        }
        if (table && !have) {
            if (int rc = w.call(cllm_op_rope_table, st, A.pos, A.hd, A.freq_base, S.cs)) return rc;
            w.tab_pos = A.pos; w.tab_hd = A.hd; w.tab_fb = A.freq_base;
        }
        // (n_kv only picks the kernel: the launch list records which one, not the length)
        return w.call(cllm_op_rope_kv_attn_decode, st, S.qkv, A.pos, table ? S.cs : nullptr, A.freq_base, w.call.sw ? (int64_t)(cllm_attn_decode_wsize(A.n_kv, A.nh, A.ML) != 0) : A.n_kv, A.nh, A.nkv, A.hd, A.mode, A.k_cache, A.v_cache, A.ML,
                      A.out, S.score_bytes ? S.scores : nullptr, S.score_bytes);
    }
    if (!A.alias) return w.call(cllm_op_attn_decode, st, A.q, A.pos, A.nh, A.nkv, A.hd, A.k_cache, A.v_cache, A.ML, A.out);
    int rc = w.call(cllm_op_attn_decode, st, A.q, A.pos, A.nh, A.nkv, A.hd, A.k_cache, A.v_cache, A.ML, S.stage);
    if (rc == CLLM_OK) rc = w.call(cllm_memcpy_d2d, (void *) A.out, (const void *) S.stage, (size_t) A.nh * A.hd * 4, st);
    return rc;
}

// one walk over the nodes; sw != nullptr: serialize the calls instead of making them
ggml_status walk(walk_ctx & w, fuse_plan & plan, sig_writer * sw) {
    w.call.sw = sw; w.merged = w.launches = 0; w.tab_pos = nullptr; w.tab_hd = 0; w.tab_fb = 0.0f;
    ggml_cgraph * g = w.g; void * st = w.st; const emitter & E = w.call;
    for (int i = 0; i < ggml_graph_n_nodes(g); i++) {
        ggml_tensor * n = ggml_graph_node(g, i);
        if (ggml_is_empty(n) || plan.skip[i]) continue;
        if (n->op == GGML_OP_NONE || n->op == GGML_OP_RESHAPE || n->op == GGML_OP_VIEW || n->op == GGML_OP_PERMUTE || n->op == GGML_OP_TRANSPOSE) continue;      // no launch
        w.launches++;
        node_io io; io.n = n; io.a = n->src[0]; io.b = n->src[1]; io.d = desc(n);
        if (io.a) io.da = desc(io.a);
        if (io.b) io.db = desc(io.b);
        cllm_tensor & d = io.d, & da = io.da, & db = io.db;
        const int alt = plan.alt[i];
        int rc = CLLM_OK;
        switch (n->op) {
            case GGML_OP_MUL_MAT:        rc = alt == ALT_FLASH_PREFILL ? issue_flash_prefill(w, plan, i, io) : plan.mv[i] >= 0 ? issue_fused_mat_vec(w, plan, i, io) : plan.pf[i] >= 0 ? issue_prefill_mat_mul(w, plan, i, io) : issue_mat_mul(w, io); break;
            case GGML_OP_MUL_MAT_ID:     rc = issue_mat_mul_id(w, io); break;
            case GGML_OP_RMS_NORM:       { float eps; memcpy(&eps, n->op_params, 4); rc = E(cllm_op_rms_norm, st, &da, &d, eps); } break;
            case GGML_OP_NORM:           { float eps; memcpy(&eps, n->op_params, 4); rc = E(cllm_op_norm, st, &da, &d, eps); } break;
            case GGML_OP_L2_NORM:        { float eps; memcpy(&eps, n->op_params, 4); rc = E(cllm_op_l2_norm, st, &da, &d, eps); } break;
            case GGML_OP_GROUP_NORM:     { float eps; memcpy(&eps, n->op_params + 1, 4); rc = E(cllm_op_group_norm, st, &da, &d, (int) n->op_params[0], eps); } break;
            case GGML_OP_ADD:            rc = alt == ALT_MOE_COMBINE ? issue_moe_combine(w, plan, i, io) : E(cllm_op_add, st, &da, &db, &d); break;
            case GGML_OP_MUL:            rc = issue_mul(w, plan, i, io); break;
            case GGML_OP_DIV:            rc = E(cllm_op_div, st, &da, &db, &d); break;
            case GGML_OP_SUM_ROWS:       rc = E(cllm_op_sum_rows, st, &da, &d); break;
            case GGML_OP_TOP_K:          rc = alt == ALT_MOE_ROUTER ? issue_moe_router(w, plan, i, io) : E(cllm_op_top_k, st, &da, &d); break;
            case GGML_OP_SCALE:          { float s, bias; memcpy(&s, n->op_params, 4); memcpy(&bias, (const float *) n->op_params + 1, 4); rc = E(cllm_op_scale, st, &da, &d, s, bias); } break;
            case GGML_OP_DIAG_MASK_INF:  rc = E(cllm_op_diag_mask_inf, st, &da, &d, n->op_params[0]); break;
            case GGML_OP_UNARY:          rc = E(cllm_op_unary, st, (int) ggml_get_unary_op(n), &da, &d); break;      // cllm_unary == ggml_unary_op
            case GGML_OP_SQR:            rc = E(cllm_op_sqr, st, &da, &d); break;
            case GGML_OP_ROPE:           rc = issue_rope(w, io); break;
            case GGML_OP_SOFT_MAX:       rc = issue_soft_max(w, plan, i, io); break;
            case GGML_OP_SET_ROWS:       rc = E(cllm_op_set_rows, st, &da, &db, &d); break;          // dst is a view of the cache (node->data)
            case GGML_OP_FLASH_ATTN_EXT: rc = issue_flash_attn_ext(w, io); break;
            case GGML_OP_CPY: case GGML_OP_DUP: case GGML_OP_CONT: rc = plan.attn[i] >= 0 ? issue_attention(w, plan, i) : E(cllm_op_cpy, st, &da, &d); break;
            case GGML_OP_GET_ROWS:       rc = E(cllm_op_get_rows, st, &da, &db, &d); break;
            case GGML_OP_IM2COL:         { const int32_t * q = n->op_params; rc = E(cllm_op_im2col, st, &da, &db, &d, (int) q[0], (int) q[1], (int) q[2], (int) q[3], (int) q[4], (int) q[5], (int) q[6]); } break;
            case GGML_OP_POOL_1D:        { const int32_t * q = n->op_params; rc = E(cllm_op_pool_1d, st, (int) q[0], &da, &d, (int) q[1], (int) q[2], (int) q[3]); } break;      // cllm_pool == ggml_op_pool
            case GGML_OP_POOL_2D:        { const int32_t * q = n->op_params; rc = E(cllm_op_pool_2d, st, (int) q[0], &da, &d, (int) q[1], (int) q[2], (int) q[3], (int) q[4], (int) q[5], (int) q[6]); } break;
            case GGML_OP_PAD:            { const int32_t * q = n->op_params; rc = E(cllm_op_pad, st, &da, &d, (int) q[0], (int) q[1], (int) q[2], (int) q[3], (int) q[4], (int) q[5], (int) q[6], (int) q[7]); } break;      // q[8] (circular) is 0: supports_op
            case GGML_OP_PAD_REFLECT_1D: { const int32_t * q = n->op_params; rc = E(cllm_op_pad_reflect_1d, st, &da, &d, (int) q[0], (int) q[1]); } break;
            case GGML_OP_UPSCALE:        rc = E(cllm_op_upscale, st, &da, &d, (int) n->op_params[0]); break;
            case GGML_OP_CONV_TRANSPOSE_1D: rc = E(cllm_op_conv_transpose_1d, st, &da, &db, &d, (int) n->op_params[0]); break;      // p0 == 0, d0 == 1: supports_op
            default: HIPB_LOG("graph_compute: op %s reached the device although supports_op() declined it", ggml_op_name(n->op)); return GGML_STATUS_FAILED;
        }
        if (rc != CLLM_OK) {
            HIPB_LOG("node %d (%s, '%s') failed: %s", i, ggml_op_name(n->op), n->name, cllm_last_error());
            return rc == CLLM_E_ALLOC ? GGML_STATUS_ALLOC_FAILED : GGML_STATUS_FAILED;
        }
    }
    return GGML_STATUS_SUCCESS;
}

// ---- the replay ladder of one stream: the list is serialized first (on a copy of the plan: the walk takes merge decisions); a step running ahead is resolved; else a list
//      equal to the captured one is replayed; else the second identical list in a row (from 8 calls) is captured and launched; else it is issued.  A failed capture re-plans,
//      issues, and stops trying.  CLLM_HIP_GRAPH=0: every call issued ----
ggml_status be_replay_or_issue(walk_ctx & w, fuse_plan & plan, const std::vector<hip_backend_ctx::scalar_set> & cur_sets, bool & replayed) {
    hip_backend_ctx * c = w.c; void * st = w.st;
    replayed = false;
    if (!g_opt.graph || c->graph_broken) return walk(w, plan, nullptr);
    static thread_local std::vector<uint8_t> sig;
    sig.clear();
    fuse_plan probe = plan;
    sig_writer sw{ sig };
    const bool sig_dbg = g_opt.sig_debug;
    static thread_local std::vector<size_t> marks;
    if (sig_dbg) { marks.clear(); sw.marks = &marks; }
    ggml_status rs = walk(w, probe, &sw);
    if (sig_dbg && sig != c->last_sig && sig.size() == c->last_sig.size()) {           // same shape of list, different bytes: which call, which byte?
        size_t off = 0; while (off < sig.size() && sig[off] == c->last_sig[off]) off++;
        size_t k = 0; while (k + 1 < marks.size() && marks[k + 1] <= off) k++;
        HIPB_LOG("launch list differs from the previous graph's in call %zu of %zu, byte %zu of that call", k, marks.size(), off - marks[k]);
    } else if (sig_dbg && sig != c->last_sig) HIPB_LOG("launch list differs from the previous graph's in length: %zu vs %zu bytes", sig.size(), c->last_sig.size());
    if (rs != GGML_STATUS_SUCCESS) return rs;
    const int n_calls = w.launches;
    bool ahead_hit = false;
    if (c->ahead.inflight) {                   // a step is running ahead: is it the one the host is asking for?
        const int hr = ahead_resolve(c, c->graph_exec && sig == c->graph_sig, cur_sets);
        if (hr < 0) return GGML_STATUS_FAILED;
        ahead_hit = hr == 1;
    }
    if (ahead_hit) {
        replayed = true; c->replays++;         // nothing to launch
        for (size_t k = 0; k < plan.groups.size(); k++) plan.groups[k].state = probe.groups[k].state;
    } else if (c->graph_exec && sig == c->graph_sig) {
        if (cllm_graph_launch(c->graph_exec, st) != CLLM_OK) { HIPB_LOG("graph replay failed: %s", cllm_last_error()); return GGML_STATUS_FAILED; }
        replayed = true; c->replays++;
        for (size_t k = 0; k < plan.groups.size(); k++) plan.groups[k].state = probe.groups[k].state;      // (statistics)
    } else if (n_calls >= 8 && sig == c->last_sig && cllm_graph_capture_begin(st) == CLLM_OK) {           // second time in a row: capture, then launch
        rs = walk(w, plan, nullptr);
        void * exec = nullptr;
        const int rc = cllm_graph_capture_end(st, &exec);
        if (rs != GGML_STATUS_SUCCESS) { if (exec) cllm_graph_destroy(exec); return rs; }
        if (rc != CLLM_OK || !exec) {           // nothing ran: do it the plain way, and stop trying
            HIPB_LOG("launch-list capture failed (%s): issuing the calls of every graph from now on", cllm_last_error());
            c->graph_broken = true;
            fuse_plan again = make_plan(w.g);
            patch_qkv_dst(again, w.S);
            rs = walk(w, again, nullptr);
            if (rs != GGML_STATUS_SUCCESS) return rs;
        } else {
            if (c->graph_exec) { cllm_stream_sync(st); cllm_graph_destroy(c->graph_exec); }
            c->graph_exec = exec; c->graph_sig = sig; c->captures++;
            if (cllm_graph_launch(exec, st) != CLLM_OK) { HIPB_LOG("graph launch failed: %s", cllm_last_error()); return GGML_STATUS_FAILED; }
        }
    } else {
        rs = walk(w, plan, nullptr);
        if (rs != GGML_STATUS_SUCCESS) return rs;
    }
    c->last_sig.swap(sig);
    return GGML_STATUS_SUCCESS;
}

void report_stats(ggml_backend_t backend, hip_backend_ctx * c, ggml_cgraph * g, const fuse_plan & plan, int launches, bool replayed) {
    int a1 = 0, a2 = 0;
    for (const fused_attn & A : plan.attns) (A.level == 2 ? a2 : a1)++;
    for (const merge_group & G : plan.groups) if (G.state == 1) launches -= G.n - 1;
    int merged_n = 0;
    for (const merge_group & G : plan.groups) merged_n += G.state == 1;
    int fa_nodes = 0;
    for (int i = 0; i < ggml_graph_n_nodes(g); i++) fa_nodes += ggml_graph_node(g, i)->op == GGML_OP_FLASH_ATTN_EXT;
    HIPB_LOG("%s graph_compute: %d nodes -> %d calls%s (%d fused mat-vecs, %d merged over packed weights, attention fused at level 1: %d, level 2: %d, flash prefill: %d, flash_attn_ext: %d, MoE routers: %d, prefill mat-muls with fused prologue / epilogue: %d)",
             be_name(backend), ggml_graph_n_nodes(g), launches, replayed ? ", replayed from the captured graph" : "", (int) plan.mvs.size(), merged_n, a1, a2, (int) plan.fas.size(), fa_nodes,
             (int) plan.routers.size(), (int) plan.pfs.size());
    g_ws.calls += launches;
    if (++g_ws.graphs % 64 == 0) {
        const double n = 64.0;
        HIPB_LOG("per graph over the last 64: host %.0f us | graph_compute %.0f us (of which planning %.0f us, %.0f calls) | synchronize %.0f us (%.1f calls) | "
                 "set_tensor %.0f us (%.1f calls) | get_tensor %.0f us (%.1f calls) | buffer alloc/free %.0f us (%.2f calls)",
                 g_ws.host_us / n, g_ws.issue_us / n, g_ws.plan_us / n, g_ws.calls / n, g_ws.sync_us / n, g_ws.syncs / n, g_ws.set_us / n, g_ws.sets / n, g_ws.get_us / n, g_ws.gets / n,
                 g_ws.alloc_us / n, g_ws.allocs / n);
        HIPB_LOG("launch lists replayed from a captured graph so far: %ld (captures: %ld); steps started ahead of the host: %ld, of which the host then asked for: %ld", c->replays, c->captures, c->ahead.launched, c->ahead.hits);
        g_ws.host_us = g_ws.plan_us = g_ws.issue_us = g_ws.sync_us = g_ws.set_us = g_ws.get_us = g_ws.alloc_us = 0; g_ws.calls = g_ws.sets = g_ws.gets = g_ws.allocs = g_ws.syncs = 0;
    }
}

ggml_status be_graph_compute(ggml_backend_t backend, ggml_cgraph * g) {
    auto * c = (hip_backend_ctx *) backend->context;
    cllm_set_device(c->device);
    if (c->kernel_error) return GGML_STATUS_FAILED;            // (an earlier launch's in-kernel wait timed out: be_sync)
    if (g_opt.trace) trace_graph(g);
    ws_scope ws(g_ws.issue_us);
    flush_sets();                               // queued small set_tensor copies (null stream; this stream does not wait for it by itself)
    cllm_set_device(c->device);
    std::vector<hip_backend_ctx::scalar_set> cur_sets;
    { std::lock_guard<std::mutex> lock(g_ring.m); if (c->device < 64) cur_sets.swap(g_scalar_sets[c->device]); }
    if (!settle_foreign_ahead(c, cur_sets)) return GGML_STATUS_FAILED;
    c->ahead.graphs++;
    fuse_plan plan = make_plan(g);
    if (g_tp.n > 1) {
        // the logical tensor-parallel device: a recognised decode step runs sharded over the ranks (tp_graph_compute); anything else runs below, un-sharded on rank 0 -- and may
        // write the KV caches behind the shards' back
        bool tp_replayed = false;
        const ggml_status ts = tp_graph_compute(c, g, plan, cur_sets, &tp_replayed);
        if (ts != GGML_STATUS_ABORTED) {
            c->last_sig.clear();
            if (ts == GGML_STATUS_SUCCESS) ahead_arm(c, g, plan, cur_sets, tp_replayed, true);      // the next sharded step may start ahead of the host, as on one device
            return ts;
        }
        if (c->ahead.inflight && c->ahead.tp) {       // a sharded step runs ahead and the host asks for something else (a prompt, another model): let it finish, put the host's scalars in place
            if (ahead_resolve(c, false, cur_sets) < 0) return GGML_STATUS_FAILED;
        }
        g_tp_kv_epoch++; g_tp.plain++; g_tp.last_tp = false; g_tp.rp.valid = false;
    }
    if (g_opt.trace) trace_plan(g, plan);
    if (g_opt.stats) g_ws.plan_us += wall_stats::us(ws.t0, wall_stats::clk::now());
    fusion_scratch S = fusion_scratch_sizes(g, plan);
    if (S.needed()) {
        if (int rc = ensure_abuf(c, S.total())) { HIPB_LOG("fusion scratch: %s", cllm_last_error()); return rc == CLLM_E_ALLOC ? GGML_STATUS_ALLOC_FAILED : GGML_STATUS_FAILED; }
        fusion_scratch_bind(S, c->abuf);
        patch_qkv_dst(plan, S);
    }
    resolve_moe_gate_up(c, g, plan);
    walk_ctx w{ c, g, c->stream, S };
    bool replayed = false;
    const ggml_status rs = be_replay_or_issue(w, plan, cur_sets, replayed);
    if (rs != GGML_STATUS_SUCCESS) return rs;
    ahead_arm(c, g, plan, cur_sets, replayed && c->graph_exec != nullptr, false);
    if (g_opt.stats) report_stats(backend, c, g, plan, w.launches, replayed);
    return GGML_STATUS_SUCCESS;       // asynchronous: the host calls synchronize() before it reads (src/backend.cpp:824-825)
}

// ---- events and the asynchronous copy between two backends of this module (ggml-backend-impl.h:87-127).  The scheduler uses them for the
//      activations that cross a layer split (`-ngl 0:40;1:40`, ggml-backend.cpp:414-433, 1473-1477): without them it synchronizes both devices and
//      goes through the blocking buffer copy at every boundary. ----
bool be_is_ours(ggml_backend_t b);
void be_event_record(ggml_backend_t b, ggml_backend_event_t e) {
    auto * c = (hip_backend_ctx *) b->context; cllm_set_device(c->device);
    if (cllm_event_record(e->context, c->stream) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] event_record failed: %s\n", cllm_last_error());
}
void be_event_wait(ggml_backend_t b, ggml_backend_event_t e) {
    auto * c = (hip_backend_ctx *) b->context; cllm_set_device(c->device);
    if (cllm_stream_wait_event(c->stream, e->context) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] event_wait failed: %s\n", cllm_last_error());
}
// src is complete once everything queued on backend_src so far has run; backend_dst must not touch dst before the copy has landed:
// the copy goes on the SOURCE stream, an event recorded behind it is what the destination stream waits for.
bool be_cpy_tensor_async(ggml_backend_t bs, ggml_backend_t bd, const ggml_tensor * src, ggml_tensor * dst) {
    if (!be_is_ours(bs) || !be_is_ours(bd) || !src->buffer || !dst->buffer || src->buffer->iface.get_base != buf_base || dst->buffer->iface.get_base != buf_base) return false;
    if (!ggml_is_contiguous(src) || !ggml_is_contiguous(dst) || ggml_nbytes(src) != ggml_nbytes(dst)) return false;
    auto * cs = (hip_backend_ctx *) bs->context; auto * cd = (hip_backend_ctx *) bd->context;
    auto * xs = (hip_buffer_ctx *) src->buffer->context; auto * xd = (hip_buffer_ctx *) dst->buffer->context;
    if (xs->device != cs->device || xd->device != cd->device) return false;       // (a tensor living on a third device: the blocking path)
    flush_sets();                                  // staged host writes to either tensor are ordered before the copy
    xd->gen++; g_tp_kv_epoch++;
    { std::lock_guard<std::mutex> lock(g_ring.m); i32_forget(dst->data, ggml_nbytes(dst)); }
    cllm_set_device(cs->device);
    if (cllm_memcpy_peer_async(dst->data, cd->device, src->data, cs->device, ggml_nbytes(src), cs->stream) != CLLM_OK) { GGML_LOG_ERROR("[ggml-hip] cpy_tensor_async ('%s' -> '%s') failed: %s\n", src->name, dst->name, cllm_last_error()); return false; }
    if (bs != bd) {
        if (!cs->copy_event) { if (cllm_event_create(&cs->copy_event) != CLLM_OK) { cs->copy_event = nullptr; cllm_stream_sync(cs->stream); return true; } }
        if (cllm_event_record(cs->copy_event, cs->stream) != CLLM_OK) { cllm_stream_sync(cs->stream); return true; }
        cllm_set_device(cd->device);
        if (cllm_stream_wait_event(cd->stream, cs->copy_event) != CLLM_OK) { cllm_set_device(cs->device); cllm_stream_sync(cs->stream); }
    }
    return true;
}
const ggml_backend_i k_backend_i = {
    be_name, be_free,
    nullptr, nullptr,                   // set/get_tensor_async: the buffer calls stage through the pinned ring already
    be_cpy_tensor_async,
    be_sync,
    nullptr, nullptr, nullptr, nullptr, // graph plans
    be_graph_compute,
    be_event_record, be_event_wait,
    nullptr,                            // graph_optimize
};
bool be_is_ours(ggml_backend_t b) { return b && b->iface.get_name == be_name; }
ggml_guid k_guid = { 0x63, 0x6c, 0x6c, 0x6d, 0x2d, 0x68, 0x69, 0x70, 0x2d, 0x67, 0x66, 0x78, 0x39, 0x35, 0x30, 0x01 };

// ---------------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------------
const char * dev_name(ggml_backend_dev_t d) { return ((hip_device_ctx *) d->context)->name.c_str(); }
const char * dev_desc(ggml_backend_dev_t d) { return ((hip_device_ctx *) d->context)->desc.c_str(); }
void dev_memory(ggml_backend_dev_t d, size_t * free, size_t * total) { cllm_device_info(((hip_device_ctx *) d->context)->id, nullptr, 0, free, total, nullptr); }
enum ggml_backend_dev_type dev_type(ggml_backend_dev_t) { return GGML_BACKEND_DEVICE_TYPE_GPU; }
void dev_props(ggml_backend_dev_t d, ggml_backend_dev_props * p) {
    p->name = dev_name(d); p->description = dev_desc(d); p->type = GGML_BACKEND_DEVICE_TYPE_GPU; p->device_id = nullptr;
    dev_memory(d, &p->memory_free, &p->memory_total);
    p->caps = { /*async*/ true, /*host_buffer*/ false, /*buffer_from_host_ptr*/ false, /*events*/ true };
}
ggml_backend_t dev_init(ggml_backend_dev_t d, const char *) {
    auto * dc = (hip_device_ctx *) d->context;
    if (cllm_set_device(dc->id)) { HIPB_LOG("set_device failed: %s", cllm_last_error()); return nullptr; }
    auto * c = new hip_backend_ctx{ dc->id };
    if (cllm_stream_create(&c->stream)) { HIPB_LOG("stream_create failed: %s", cllm_last_error()); delete c; return nullptr; }
    return new ggml_backend{ &k_guid, k_backend_i, d, c };
}
ggml_backend_buffer_type_t dev_buft(ggml_backend_dev_t d) { return &((hip_device_ctx *) d->context)->buft; }
bool dev_supports_buft(ggml_backend_dev_t d, ggml_backend_buffer_type_t t) { return t->iface.get_name == buft_name && t->context == d->context; }
ggml_backend_event_t dev_event_new(ggml_backend_dev_t d) {
    cllm_set_device(((hip_device_ctx *) d->context)->id);
    void * e = nullptr;
    if (cllm_event_create(&e) != CLLM_OK) { GGML_LOG_ERROR("[ggml-hip] event_new failed: %s\n", cllm_last_error()); return nullptr; }
    return new ggml_backend_event{ d, e };
}
void dev_event_free(ggml_backend_dev_t, ggml_backend_event_t e) { if (e) { cllm_event_destroy(e->context); delete e; } }
void dev_event_synchronize(ggml_backend_dev_t, ggml_backend_event_t e) { if (cllm_event_sync(e->context) != CLLM_OK) GGML_LOG_ERROR("[ggml-hip] event_synchronize failed: %s\n", cllm_last_error()); }
const ggml_backend_device_i k_device_i = {
    dev_name, dev_desc, dev_memory, dev_type, dev_props, dev_init, dev_buft,
    nullptr, nullptr,                   // host buffer type, buffer_from_host_ptr (SURVEY.md 8b note: keep NULL)
    dev_supports_op, dev_supports_buft,
    nullptr,                            // offload_op
    dev_event_new, dev_event_free, dev_event_synchronize,
};
std::vector<ggml_backend_device> g_dev_objs;

// ---------------------------------------------------------------------------------------------------------------------------
// reg
// ---------------------------------------------------------------------------------------------------------------------------
const char * reg_name(ggml_backend_reg_t) { return "HIP"; }
size_t reg_count(ggml_backend_reg_t) { return g_dev_objs.size(); }
ggml_backend_dev_t reg_get(ggml_backend_reg_t, size_t i) { return i < g_dev_objs.size() ? &g_dev_objs[i] : nullptr; }
void * reg_proc(ggml_backend_reg_t, const char *) { return nullptr; }
const ggml_backend_reg_i k_reg_i = { reg_name, reg_count, reg_get, reg_proc };

}  // namespace

extern "C" {
GGML_BACKEND_API ggml_backend_reg_t ggml_backend_init(void);
GGML_BACKEND_API int ggml_backend_score(void);
}

ggml_backend_reg_t ggml_backend_init(void) {
    static std::once_flag once;
    std::call_once(once, [] {
        // CLLM_HIP_VIRTUAL_DEVICES=n: register n ggml devices over the physical ones (device i runs on GPU i % physical) -- the reference's own multi-device modes
        // (layer split `-ngl "0:16;1:16"`, src/backend.cpp:677-778: a buffer type, a backend, a stream per device; activations cross through cpy_tensor_async +
        // events) then run through the real scheduler on a one-GPU box.  Each ggml device has its own buffer type, so tensors of device 1 are foreign to device 0
        // exactly as on two GPUs; what the physical sharing changes is only that the "peer" copy stays inside one HBM.
        g_opt.read();
        const int phys = cllm_device_count();
        int n = phys;
        if (g_opt.virtual_devices > 0 && phys > 0) n = g_opt.virtual_devices;      // (at most 64: the table clamps)
        // CLLM_HIP_TP=N: ONE logical device over N tensor-parallel ranks (rank r on GPU r % physical: more ranks than GPUs = virtual ranks sharing a GPU) -- tp_graph_compute
        if (g_opt.tp > 1 && phys > 0) { g_tp.n = g_opt.tp; n = 1; }      // (at most 16: the table clamps)
        g_dev_objs.reserve(n);
        for (int i = 0; i < n; i++) {
            auto * d = new hip_device_ctx();
            char name[256] = "MI355X"; int cus = 0;
            const int gpu = i % phys;
            cllm_device_info(gpu, name, sizeof(name), nullptr, nullptr, &cus);
            d->id = gpu; d->name = "HIP" + std::to_string(i); d->desc = std::string(name) + ", " + std::to_string(cus) + " CUs (chatllm.cpp_amd" + (n != phys ? ", GPU " + std::to_string(gpu) : std::string()) +
                      (g_tp.n > 1 ? ", tensor parallel over " + std::to_string(g_tp.n) + " ranks on " + std::to_string(g_tp.n < phys ? g_tp.n : phys) + " GPU(s)" : std::string()) + ")";
            g_devices.push_back(d);
            g_dev_objs.push_back(ggml_backend_device{ k_device_i, &g_reg, d });
            d->buft = ggml_backend_buffer_type{ k_buft_i, &g_dev_objs.back(), d };
        }
        g_reg = ggml_backend_reg{ GGML_BACKEND_API_VERSION, k_reg_i, nullptr };
    });
    return &g_reg;
}
int ggml_backend_score(void) { return cllm_device_count() > 0 ? 100 : 0; }
