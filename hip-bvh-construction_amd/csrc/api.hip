// api.hip — the C ABI of include/bvh_mi355x.h: context/arena management and the host orchestration of the build
// (what X::build does in the reference: src/TwoPassLbvh.cpp:17-197, src/SinglePassLbvh.cpp:17-188,
// src/PLOC++Bvh.cpp:16-196, src/Hploc.cpp:16-165 — minus RTC compilation, per-call allocation and debug read-backs).
#include <hip/hip_runtime.h>
#include <new>
#include <cstring>
#include <cstdlib>
#include "bvh_mi355x.h"
#include <mutex>
#include "common.hpp"
#include "kernels.hpp"

#include <vector>
#include <string>
#include <map>

using namespace bvh;

namespace bvh { thread_local KernelRecorder* g_recorder = nullptr; }

struct EventRecorder : KernelRecorder {
    struct Rec { const char* name; hipEvent_t ev; };
    std::vector<Rec> recs; size_t used = 0;
    std::string only;                 // non-empty: record this kernel's marks only (and the mark that closes each of its intervals)
    bool open = false;
    void mark(hipStream_t s, const char* name) override {
        if (!only.empty()) {
            const bool match = name && only == name;
            if (!match && !open) return;          // an event costs ~5 us of launch gap: a build is 7 launches
            if (!match) name = nullptr;           // closes the interval of the watched kernel
            open = match;
        }
        if (used == recs.size()) { Rec r{name, nullptr}; if (hipEventCreate(&r.ev) != hipSuccess) return; recs.push_back(r); }
        recs[used].name = name; (void)hipEventRecord(recs[used].ev, s); ++used;
    }
    void reset() { used = 0; open = false; }
    ~EventRecorder() override { for (auto& r : recs) if (r.ev) (void)hipEventDestroy(r.ev); }
};

struct bvh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool profiling = false;           // stage-level events (the reference's Timer tokens)
    bool kernel_profiling = false;    // + one event pair per kernel launch
    uint32_t sample_every = 1, build_counter = 0;   // ... of every sample_every-th build only
    EventRecorder recorder;
    uint32_t cap = 0;                 // primitives the arena is sized for
    char* arena = nullptr;
    size_t arena_bytes = 0;
    // carved from the arena
    void* tris = nullptr;             // Triangle[cap] staging for host inputs (allocated lazily, separate)
    uint32_t tris_cap = 0;
    bvh_aabb* boxes = nullptr;
    float* scene = nullptr;
    u32 *keys = nullptr, *skeys = nullptr, *svals = nullptr;   // keys / skeys: 8 bytes per primitive (u32 keys use the first half)
    SortScratch sort{};
    bvh2_node* nodes = nullptr;       // 2*cap
    bvh_primref* leaves = nullptr;    // cap
    u64* slots = nullptr;             // cap           (u64 scratch: BVH4 collapse task queue)
    u32* parent = nullptr;            // 2*cap         (two-pass parent pointers / HPLOC parentIdx)
    u32* flags = nullptr;             // cap           (two-pass refit exchange words: all-INVALID, kept so by the protocol)
    HplocScratch hploc{};             //               (hploc.dep is zeroed when the arena is allocated and stays clean)
    PlocScratch ploc{};
    u32* small = nullptr;             // 64 words: [0] root, [1] hploc node counter, [8..9] f64 SAH
    u64* overlap_sums = nullptr;      // OVERLAP_SCAN_BLOCKS  (bvh_overlap's scan: chunk sums)
    size_t lbvh_queue_capacity = 0;   // uint4 entries of ploc.list0 (>= kernels.hpp lbvh_queue_capacity(cap))
    // The emitters' self-cleaning scratch (hploc.dep / LBVH slots all-zero, two-pass flags all-ones) is only clean after a build that ran to
    // completion.  Set while an emit is being enqueued, cleared when every launch of it was accepted: a build that failed in between
    // (HIP error, early return) makes the next one re-initialise the words instead of silently producing wrong trees.
    bool scratch_dirty = false;
    hipEvent_t ev[8] = {};
    int scene_slot = 0;               // which of the two scene extents the next build uses
    bool scene_ready = false;         // that extent holds Aabb::reset values (written by the previous build's Morton kernel); false: reset it explicitly
    uint32_t ploc_last_n = 0, ploc_last_iters = 0;   // size and iteration count of the last PLOC++ build (run_ploc aims its first batch of launches at it)
    u32* h_pinned = nullptr;          // pinned, device-accessible host words: the small read-backs (root index, PLOC++ state, collapse level counts) land here as {v, ~v} pairs
    u32* d_pinned = nullptr;          // the same words as the device addresses them
    float last_collapse_ms = 0.f;     // CollapseBvhTime of the last bvh_collapse4 (profiling on)
    uint32_t collapse_last_n = 0, collapse_last_levels = 0;   // levels the previous collapse of a tree of this size needed (first batch of launches)
    uint64_t collapse_last_key = 0;                           // ... of this KIND: {node layout, root index} — an LBVH and a PLOC tree of one size have different level widths
    uint32_t collapse_last_len[COLLAPSE_MAX_BATCH] = {0};     // ... and their task counts (grid sizes of the first batch's launches),
    int collapse_len_batch = 0;                               //     valid for that many levels (0: the previous collapse took several batches)
    int64_t options[4] = {0, 0, 0, 0}; // bvh_option values (bvh_ctx_set_option); all default 0 = decide by input size / no test knobs
    // bvh_refit's parent plan of the ctx's own tree, kept in `parent` while nothing rewrote nodes / leaves / parent: every path that writes them (a build, the
    // bvh_emit_* entry points, a re-allocation, the device-memory helpers, which may be aimed at the arena) bumps tree_serial; the plan is valid for
    // {plan_serial == tree_serial, plan_n, plan_root}.  plan_serial 0: no plan (a refit of caller-owned arrays made one of ITS tree in `parent`).
    uint64_t tree_serial = 1, plan_serial = 0;
    uint32_t plan_n = 0, plan_root = 0;
    // bvh_refit_subset's words, outside the arena (a build's footprint and the emitters' scratch protocols do not change): leaf_of_prim | owner | pending, u32[subset_cap]
    // each, allocated by the first bvh_refit_subset and again after the capacity grew.  owner / pending are zeroed once and kept all-zero by a completed call;
    // subset_dirty: set while a call is being enqueued and left set by a call on caller-owned arrays (not a tree: marks can stay behind); the next call zeroes
    // the words first, whichever tree it is on (as scratch_dirty).  The leaf map of the
    // ctx's own tree is kept under the plan's rule: valid for {map_serial == tree_serial, map_n, map_root}; bvh_optimize moves no leaf and leaves it valid.
    u32* subset_words = nullptr;
    uint32_t subset_cap = 0;
    bool subset_dirty = false;
    uint64_t map_serial = 0;
    uint32_t map_n = 0, map_root = 0;
    // bvh_split_refs' words, outside the arena (the call needs no tree and must not move one): u64 total | u32 heavy count | (pad to 64 bytes) |
    // u64 scan sums[OVERLAP_SCAN_BLOCKS] | u32 heavy list[split_cap].  Calls on the ctx's stream are ordered, so one set serves them all
    char* split_words = nullptr;
    uint32_t split_cap = 0;
    // bvh_build_many's item table, outside the arena (the call may not touch it): uint4 {first, count, out_off, mesh} per mesh, binned by size class.  The host fills the
    // pinned copy and an asynchronous copy on the stream brings it over; many_ev marks the end of that copy, so the next call knows when it may refill the pinned words
    uint4* many_items = nullptr;
    uint4* many_host = nullptr;
    uint32_t many_cap = 0;
    hipEvent_t many_ev = nullptr;
};

// bvh_scene: device memory of its own (one allocation, carved as below), outside the ctx's arena; only the top-level build uses the arena
struct bvh_scene {
    bvh_ctx* ctx = nullptr;
    char* mem = nullptr;
    bool built = false;
    uint32_t n_blas = 0, n_inst = 0, troot = 0, tlayout = 0;
    bvh::SceneBlas* blas = nullptr;    // [n_blas] device copies of the validated descriptors
    bvh_instance* inst_in = nullptr;   // [n_inst] the caller's instance records
    bvh::SceneInst* inst = nullptr;    // [n_inst] world-to-object + active flag (k_instance_boxes)
    bvh_aabb* wbox = nullptr;          // [n_inst] world boxes by instance index (the top-level tree's primitive boxes)
    bvh2_node* tnodes = nullptr;       // top-level tree: layout 0 2n-1 nodes, layout 1 n-1 nodes + n leaves (n_inst >= 2)
    bvh_primref* tleaves = nullptr;
    u32* tparent = nullptr;            // [2n-1] top-level plan
    u32* flags = nullptr;              // [n] refit exchange words (all-INVALID, kept so)
    u32* overflow = nullptr;           // [1] rays left to the stackless pass
    // winding numbers (bvh_scene_winding_prepare): an allocation of its own, made by the first prepare after a build and freed by the next build
    std::vector<uint32_t> blas_n;      // the BLASes' leaf counts (host): the prefix table is made from them at prepare time
    char* wmem = nullptr;
    bvh::SceneWind wind{};
    bool wind_blas_ok = false;         // the BLAS moments were made since the last bvh_scene_build
    bool wind_ok = false;              // ... and the maps, instance moments and top-level moments since the last build or update
};

namespace {

// HPLOC: one asynchronous launch below this size, LDS-tiled block kernel + external climb above (measured on MI355X: 1122 vs 966
// Mtris/s at 262 k, 3005 vs 3416 at 2 M, 3848 vs 5616 at 10 M; whole build, one launch / tiles, end of round 3 (tools/ab_sched_small.py):
// 400 k 0.1928 / 0.2302 ms, 600 k 0.2134 / 0.2234, 900 k 0.2603 / 0.2511)
constexpr uint32_t HPLOC_BLOCK_MIN_N = 800000;
inline bool hploc_use_block(const bvh_ctx* c, uint32_t n) {
    if (n <= 2 * hploc_block_tile()) return false;     // the root must cross tiles
    const int64_t o = c->options[BVH_OPT_HPLOC_SCHEDULER];   // 1 async / 2 tiles: the host's override (A/B measurements, tests)
    if (o == 1) return false;
    if (o == 2) return true;
    return n >= HPLOC_BLOCK_MIN_N;
}
// HPLOC emit on the ctx's scratch (SetupClusters + HPloc, src/Hploc.cpp:83-121)
void emit_hploc(bvh_ctx* c, hipStream_t s, const void* d_boxes, const void* d_skeys, int key_bits, const u32* d_svals, uint32_t n, void* d_nodes, void* d_leaves,
                bool heads_cleared = false) {
    if (hploc_use_block(c, n)) launch_hploc_block(s, d_boxes, d_skeys, key_bits, d_svals, n, d_nodes, d_leaves, c->hploc, heads_cleared);
    else launch_hploc(s, d_boxes, d_skeys, key_bits, d_svals, n, d_nodes, d_leaves, c->hploc);
}

inline int herr(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return -(int)_e; } while (0)

// The per-build read-backs (single-pass LBVH root index, PLOC++ iteration state, the collapse's level counts) are a handful of words.  They come back as PAIRS
// {v, ~v} written by a one-workgroup kernel straight into pinned, device-accessible host words (misc.hip launch_readback); the caller arms every pair with
// {sentinel, sentinel} — an inconsistent pair — and wait_readback polls until EVERY pair reads {v, ~v}: hipStreamSynchronize notices the end of the stream ~6 us later
// than a poll of the words does (tools/probes/sync_latency.hip), 4 % of a 262 144-triangle LBVH build.  A consistent pair proves that every byte of both words is final:
// no assumption about the order or the granularity in which a copy becomes visible to the host (round 3 polled the last word of a hipMemcpyAsync for "not the
// sentinel" — ADVICE r03 —, and round 4 caught that copy landing byte by byte: see misc.hip).  Acquire loads: nothing read afterwards can be hoisted above the poll.  The
// stream is in order, so everything enqueued before the read-back kernel is complete when the pairs are.  Bounded: after ~4 M rounds it falls back to hipStreamSynchronize,
// which also surfaces an error of the stream.
static int wait_readback(hipStream_t s, const u32* pairs, u32 count) {
    auto all_landed = [&]() -> bool {
        for (u32 i = 0; i < count; ++i) {
            const u32 v = __atomic_load_n(pairs + 2 * i, __ATOMIC_ACQUIRE), w = __atomic_load_n(pairs + 2 * i + 1, __ATOMIC_ACQUIRE);
            if (w != ~v) return false;
        }
        return true;
    };
    for (u32 polls = 0; polls < (1u << 22); ++polls) {
        if (all_landed()) return 0;
#if defined(__x86_64__)
        __builtin_ia32_pause();                      // (be a polite spinner: the runtime's helper threads may share this core)
#endif
    }
    HIP_TRY(hipStreamSynchronize(s));
    return all_landed() ? 0 : BVH_E_INTERNAL;
}
static inline void arm_readback(u32* pairs, u32 count) {
    for (u32 i = 0; i < 2 * count; ++i) __atomic_store_n(pairs + i, 0xFFFFFFFFu, __ATOMIC_RELAXED);      // {S, S}: never a consistent pair
    __atomic_thread_fence(__ATOMIC_RELEASE);
}
// enqueue the read-back of na words at d_a and nb words at d_b behind everything on the stream and wait for it; the values are then pairs[2 i]
static int read_back(bvh_ctx* c, const u32* d_a, u32 na, const u32* d_b, u32 nb, u32* pairs);

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct Carver {
    char* base; size_t off = 0;
    template <typename T> T* take(size_t count) { T* p = base ? reinterpret_cast<T*>(base + off) : nullptr; off += align_up(count * sizeof(T)); return p; }
};

void carve(bvh_ctx* c, char* base, uint32_t cap, size_t* total) {
    Carver k{base};
    const size_t n = cap;
    c->boxes = k.take<bvh_aabb>(n);
    c->scene = k.take<float>(16);          // two extents of 8 floats: builds alternate, the Morton kernel of one build resets the other for the next
    c->keys = reinterpret_cast<u32*>(k.take<u64>(n)); c->skeys = reinterpret_cast<u32*>(k.take<u64>(n)); c->svals = k.take<u32>(n);
    c->sort.pairs0 = k.take<uint4>(n); c->sort.pairs1 = k.take<uint4>(n);
    c->sort.hist = k.take<u32>(SORT_HIST_COPIES * SORT_HIST_STRIDE);
    c->sort.status = k.take<u32>(sort_status_bytes(cap) / sizeof(u32));
    c->sort.counters = k.take<u32>(SORT_MAX_PASSES);
    c->nodes = k.take<bvh2_node>(2 * n);
    c->leaves = k.take<bvh_primref>(n);
    c->slots = k.take<u64>(n);
    c->parent = k.take<u32>(2 * n);
    c->flags = k.take<u32>(n);
    c->hploc.recs = k.take<bvh2_node>(n);
    c->hploc.dep = k.take<u64>(n);
    c->hploc.queue_capacity = hploc_queue_capacity(cap);
    c->hploc.queue_pc = k.take<u32>(c->hploc.queue_capacity);
    c->hploc.queue_rng = k.take<u64>(c->hploc.queue_capacity);
    c->hploc.queue_count = k.take<u32>(hploc_head_words());  // (one padded head per sub-queue)
    c->lbvh_queue_capacity = 2 * n > lbvh_queue_capacity(cap) ? 2 * n : lbvh_queue_capacity(cap);   // list0 doubles as the LBVH tile scheduler's root queue
    c->ploc.list0 = k.take<uint4>(c->lbvh_queue_capacity);
    c->ploc.list1 = k.take<uint4>(2 * n);
    c->ploc.ids1 = k.take<u32>(n);
    c->ploc.status = k.take<u64>((size_t)PLOC_MAX_ITERS * ploc_chunks(cap));
    c->ploc.state = k.take<u32>(PLOC_STATE_WORDS);
    c->small = k.take<u32>(64);            // [0] root, [1] hploc zero-parent, [8..9] f64 SAH / BVH4 cost, [10..11] u64 checksum, [16..31] camera, [32..47] transform, [48..57] Morton plan read-back, [58..63] the query calls' words (overflow_words / total_word / rows_word below)
    c->hploc.zero_parent = c->small + 1;
    c->overlap_sums = k.take<u64>(OVERLAP_SCAN_BLOCKS);
    *total = k.off;
}
// The query calls' words.  Every tree query and every count -> scan -> fill scene query of a ctx shares them (query_tail, count_fill_tail below; bvh_split_refs
// shares the pinned pairs): calls on one stream are ordered, so a call's kernels and its read-back are done with the words before the next call's memset runs.
inline u32* overflow_words(const bvh_ctx* c) { return c->small + 58; }                            // queries left to the stackless pass: [0] single pass / count pass, [1] fill pass
inline u64* total_word(const bvh_ctx* c) { return reinterpret_cast<u64*>(c->small + 60); }        // the count pass's u64 total (small[60..61])
inline u64* rows_word(const bvh_ctx* c) { return reinterpret_cast<u64*>(c->small + 62); }         // bvh_scene_collide's u64 n_rows (small[62..63]): it survives the count pass's scan, which writes total_word
inline u32* total_pairs(const bvh_ctx* c) { return c->h_pinned + 8; }                             // {lo, ~lo, hi, ~hi} of a total read back: pinned words 8..11

int ensure_capacity(bvh_ctx* c, uint32_t n) {
    if (n <= c->cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->arena) { HIP_TRY(hipFree(c->arena)); c->arena = nullptr; c->cap = 0; }
    size_t total = 0;
    carve(c, nullptr, n, &total);
    char* p = nullptr;
    HIP_TRY(hipMalloc(&p, total));
    c->arena = p; c->arena_bytes = total; c->cap = n;
    ++c->tree_serial;
    c->scene_ready = false; c->scene_slot = 0;
    carve(c, p, n, &total);
    HIP_TRY(hipMemsetAsync(c->hploc.dep, 0, (size_t)n * sizeof(u64), c->stream));   // HPLOC dependency words: clean once, builds keep them clean
    HIP_TRY(hipMemsetAsync(c->flags, 0xFF, (size_t)n * sizeof(u32), c->stream));    // two-pass LBVH exchange words: likewise
    return 0;
}

// re-initialise the self-cleaning emit scratch after a build that did not run to completion (see bvh_ctx::scratch_dirty)
int begin_emit(bvh_ctx* c) {
    if (c->scratch_dirty) {
        HIP_TRY(hipMemsetAsync(c->hploc.dep, 0, (size_t)c->cap * sizeof(u64), c->stream));
        HIP_TRY(hipMemsetAsync(c->flags, 0xFF, (size_t)c->cap * sizeof(u32), c->stream));
    }
    c->scratch_dirty = true;
    return 0;
}
int end_emit(bvh_ctx* c) {
    HIP_TRY(hipGetLastError());
    c->scratch_dirty = false;
    return 0;
}

int ensure_tris(bvh_ctx* c, uint32_t n) {
    if (n <= c->tris_cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->tris) { HIP_TRY(hipFree(c->tris)); c->tris = nullptr; c->tris_cap = 0; }
    HIP_TRY(hipMalloc(&c->tris, (size_t)n * sizeof(bvh_triangle)));
    c->tris_cap = n;
    return 0;
}

struct Bind { int prev = -1; bool ok = true;
    explicit Bind(int dev) { ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess); }
    ~Bind() { int cur; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) hipSetDevice(prev); } };

// One tick of the ctx's sampling counter (bvh_ctx_set_kernel_sampling: events in every n-th build or query only) and, while the guard lives, the ctx's kernel
// recorder installed if this call is a sampled one.  Constructed where a call starts to enqueue: after every argument check and every early return, so that a
// refused or empty call consumes no tick.  mark() closes the interval of the call's last kernel
struct Install { bvh_ctx* c; bool sampled, on;
    explicit Install(bvh_ctx* ctx) : c(ctx), sampled((ctx->build_counter++ % ctx->sample_every) == 0u), on(ctx->kernel_profiling && sampled) { if (on) g_recorder = &c->recorder; }
    void mark() const { if (on) c->recorder.mark(c->stream, nullptr); }
    void end() { if (on) g_recorder = nullptr; on = false; }
    ~Install() { end(); } };

static int read_back(bvh_ctx* c, const u32* d_a, u32 na, const u32* d_b, u32 nb, u32* pairs) {
    arm_readback(pairs, na + nb);
    launch_readback(c->stream, d_a, na, d_b, nb, c->d_pinned + (pairs - c->h_pinned));
    HIP_TRY(hipGetLastError());
    return wait_readback(c->stream, pairs, na + nb);
}
// the only wait of a count -> scan -> fill call, and only when the caller asks for the total: the u64 at d_total comes back through total_pairs
static int read_total(bvh_ctx* c, const u64* d_total, uint64_t* total_out) {
    u32* const rb = total_pairs(c);
    const int r = read_back(c, reinterpret_cast<const u32*>(d_total), 2, nullptr, 0, rb); if (r) return r;
    *total_out = (uint64_t)rb[0] | ((uint64_t)rb[2] << 32);
    return *total_out > 0xFFFFFFFFull ? BVH_E_TOO_LARGE : 0;
}

// PLOC++ iteration driver: batches of device-side iterations, one small read-back per batch (src/PLOC++Bvh.cpp:132-152
// reads back after EVERY iteration).
int run_ploc(bvh_ctx* c, uint32_t n, void* d_nodes, void* d_leaves, const void* d_boxes, const u32* d_svals, const PlocScratch& sc, uint32_t* iterations_out) {
    u32* const host_state = c->h_pinned + 16;                // (pinned: the per-batch read-back does not go through a staging buffer)
    constexpr size_t state_bytes = PLOC_STATE_WORDS * sizeof(u32);
    u32 iters_before = 0;                                    // iterations counted before the bookkeeping was last restarted (a restart clears the device's counter)
    int first = 0, parity = 0;
    bool fresh = true;
    // iterations needed grow by ~3 per doubling of n (measured: 30 at 262 k, 45 at 10 M); the first batch aims slightly above
    // (round 2: 30 at 262 k, 34 at 2 M, 40 at 10 M on uniform meshes — two more per doubling; a launch after the end still costs ~5 us)
    int batch = 32; for (uint32_t m = n; m > 262144u; m >>= 1) batch += 2; if (batch > 80) batch = 80;
    // rebuilds of a scene of the same size (animation frames; the benchmark loop) need the same number of iterations give or take one: aim one above the
    // previous build's count instead of two to four (an iteration launched after the end costs ~5 us; one short costs a read-back and a second batch)
    if (c->ploc_last_n == n && c->ploc_last_iters > 0 && c->ploc_last_iters + 1 < PLOC_MAX_ITERS) batch = (int)c->ploc_last_iters + 1;
    // every iteration merges at least the globally closest pair, so n iterations always suffice (a collinear, zero-area scene needs
    // almost that many: every union has area 0 and only the lowest pair of a chunk is mutual); the reference loops the same way
    for (uint32_t guard = 0; guard < n / 16u + 4096u; ++guard) {
        if (first + batch > PLOC_MAX_ITERS) {
            // restart the per-iteration bookkeeping with the current count (pathologically slow convergence only)
            HIP_TRY(hipMemcpyAsync(host_state, sc.state, state_bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const u32 count = host_state[first];
            iters_before += host_state[2 * PLOC_MAX_ITERS + 1];
            parity = (parity + first) & 1;
            ploc_reset(c->stream, sc, n, count);
            first = 0;
        }
        ploc_enqueue(c->stream, sc, n, d_nodes, d_leaves, d_boxes, d_svals, first, batch, parity, fresh);
        fresh = false;
        // two words come back: the iterations done so far and the cluster count after this batch (pairs at pinned words 4..7)
        u32* const rb = c->h_pinned + 4;
        { const int wr = read_back(c, sc.state + 2 * PLOC_MAX_ITERS + 1, 1, sc.state + first + batch, 1, rb); if (wr) return wr; }
        const u32* const h_iters = rb; const u32* const h_count = rb + 2;
        const u32 count = *h_count;
        if (count <= 1) {
            c->ploc_last_n = n; c->ploc_last_iters = iters_before ? 0u : *h_iters;
            if (iterations_out) *iterations_out = iters_before + *h_iters;
            return 0;
        }
        first += batch; batch = 16;
    }
    return BVH_E_INTERNAL;
}

// stage E on any of the input formats of bvh_build_input (device pointers)
int stage_extents_valid(const bvh_build_input* in) {
    switch (in->tri_format) {
        case BVH_TRI_PADDED64: return in->d_tris ? 0 : BVH_E_INVALID_ARG;
        case BVH_TRI_PACKED36: return (in->d_tris && !((uintptr_t)in->d_tris & 15u)) ? 0 : BVH_E_INVALID_ARG;      // 16-byte loads
        case BVH_TRI_INDEXED:  return (in->d_vertices && in->d_indices && in->n_vertices) ? 0 : BVH_E_INVALID_ARG;
        default: return BVH_E_INVALID_ARG;
    }
}
int stage_extents_fmt(hipStream_t s, const bvh_build_input* in, uint32_t n, void* d_boxes, void* d_scene, bool reset_scene = true, const PrepArgs* prep = nullptr) {
    const int v = stage_extents_valid(in); if (v) return v;
    switch (in->tri_format) {
        case BVH_TRI_PADDED64: launch_extents(s, in->d_tris, n, d_boxes, d_scene, reset_scene, prep); return 0;
        case BVH_TRI_PACKED36: launch_extents_packed(s, in->d_tris, n, d_boxes, d_scene, reset_scene, prep); return 0;
        case BVH_TRI_INDEXED:  launch_extents_indexed(s, in->d_vertices, in->d_indices, in->n_vertices, n, d_boxes, d_scene, reset_scene, prep); return 0;
        default: return BVH_E_INVALID_ARG;
    }
}

// what every call that walks a caller-supplied tree requires of it
inline bool tree_valid(const bvh_result* tree) {
    const uint32_t n = tree->n_leaves;
    return !(n < 2 || tree->layout > 1u || !tree->d_nodes || (tree->layout == 1u && !tree->d_leaves) || tree->root >= n - 1);
}
// the triangles a tree query reads: the caller's (validated) or the tree's own d_tris as Triangle[n]
int resolve_tris(const bvh_result* tree, const bvh_build_input* tris, bvh_build_input* in) {
    std::memset(in, 0, sizeof *in);
    if (tris) { if (stage_extents_valid(tris)) return BVH_E_INVALID_ARG; *in = *tris; }
    else { if (!tree->d_tris) return BVH_E_INVALID_ARG; in->tri_format = BVH_TRI_PADDED64; in->d_tris = tree->d_tris; }
    return 0;
}

// A byte range of memory, for the "these arrays may not overlap" checks.  A null pointer or zero bytes give an empty range, and an empty range crosses nothing.
struct Range { uintptr_t lo = 0, hi = 0;
    Range() = default;
    Range(const void* p, uint64_t bytes) : lo((uintptr_t)p), hi((uintptr_t)p + (p ? bytes : 0u)) {} };
// does a cross any of the k ranges rs?
inline bool crosses(const Range& a, const Range* rs, int k) {
    for (int i = 0; i < k; ++i) if (a.lo < a.hi && rs[i].lo < rs[i].hi && a.lo < rs[i].hi && rs[i].lo < a.hi) return true;
    return false;
}
inline bool crosses(const Range& a, const Range& b) { return crosses(a, &b, 1); }
// does none of the first m of the k ranges rs (a call's outputs) cross a range after it (m == k: are the k ranges pairwise disjoint?)
inline bool disjoint(const Range* rs, int m, int k) {
    for (int a = 0; a < m; ++a) if (crosses(rs[a], rs + a + 1, k - a - 1)) return false;
    return true;
}
// a mesh's one or two arrays of `count` triangles appended to rs; returns how many
inline int mesh_ranges(const bvh_build_input& m, uint32_t count, Range* rs) {
    if (m.tri_format != BVH_TRI_INDEXED) { rs[0] = Range(m.d_tris, (uint64_t)count * (m.tri_format == BVH_TRI_PACKED36 ? 36u : 64u)); return 1; }
    rs[0] = Range(m.d_vertices, (uint64_t)m.n_vertices * 12u); rs[1] = Range(m.d_indices, (uint64_t)count * 12u);
    return 2;
}
// a tree's node array, and its leaf array in layout 1, appended to rs; returns how many
inline int tree_ranges(const bvh_result* tree, Range* rs) {
    const uint32_t n = tree->n_leaves;
    rs[0] = Range(tree->d_nodes, (uint64_t)(tree->layout == 0u ? 2ull * n - 1 : n - 1ull) * sizeof(bvh2_node));
    if (tree->layout == 1u) rs[1] = Range(tree->d_leaves, (uint64_t)n * sizeof(bvh_primref));
    return tree->layout == 1u ? 2 : 1;
}
// the cap on what a fill pass may write: d_out is never written past 2^32 - 1 records (a larger total skips the fill)
inline Range fill_range(const void* d_out, uint64_t capacity, size_t record) { return Range(d_out, (capacity < 0xFFFFFFFFull ? capacity : 0xFFFFFFFFull) * record); }

// the stackless pass's parent plan: bvh_refit's, cached for the ctx's own tree under the same rule
void query_plan(bvh_ctx* c, const bvh_result* tree, hipStream_t s) {
    const bool own = tree->d_nodes == c->nodes;
    if (!own || c->plan_serial != c->tree_serial || c->plan_n != tree->n_leaves || c->plan_root != tree->root) {
        launch_refit_plan(s, tree->d_nodes, tree->n_leaves, tree->root, c->parent);
        c->plan_serial = own ? c->tree_serial : 0; c->plan_n = tree->n_leaves; c->plan_root = tree->root;
    }
}

// What a single-pass query does once its arguments are checked and it has queries to answer: bind, tick (Install), the parent plan of a tree query (tree: null for
// a scene query, whose plans the scene keeps), the overflow word zeroed, launch(stream, overflow).  An error that enqueuing gave is returned; a tree query then
// also drops the cached plan, which a refused launch may not have written
template <typename Launch>
int query_tail(bvh_ctx* c, const bvh_result* tree, u32* overflow, Launch launch) {
    Bind b(c->device);
    hipStream_t s = c->stream;
    Install install(c);
    if (tree) query_plan(c, tree, s);
    hipError_t e = hipMemsetAsync(overflow, 0, sizeof(u32), s);
    if (e == hipSuccess) { launch(s, overflow); e = hipGetLastError(); }
    if (e != hipSuccess) { if (tree) c->plan_serial = 0; return herr(e); }
    install.mark();
    return 0;
}

// What a count -> scan -> fill query does once its arguments are checked.  No queries: d_offsets[0] = total = 0 and nothing else, not even a tick.  Otherwise: tick,
// the parent plan of a tree query (tree: null for a scene query, which instead makes sure the arena holding the words exists), the four words zeroed,
// launch(stream, overflow, total) — the count pass and, where the caller gave an output array, the fill pass on overflow + 1 —, errors as query_tail, and the
// call's only wait: the total's read-back, when the caller asks for it
template <typename Launch>
int count_fill_tail(bvh_ctx* c, const bvh_result* tree, uint32_t n_queries, uint32_t* d_offsets, uint64_t* total_out, Launch launch) {
    Bind b(c->device);
    hipStream_t s = c->stream;
    if (n_queries == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(u32), s));
        if (total_out) *total_out = 0;
        return 0;
    }
    Install install(c);
    if (tree) query_plan(c, tree, s);
    // (a one-instance scene on a fresh ctx never made the arena — no top-level build: the smallest one, nothing points into it)
    else if (!c->arena) { const int r = ensure_capacity(c, 2); if (r) return r; }
    u32* const overflow = overflow_words(c);
    u64* const total = total_word(c);
    hipError_t e = hipMemsetAsync(overflow, 0, 4 * sizeof(u32), s);
    if (e == hipSuccess) { launch(s, overflow, total); e = hipGetLastError(); }
    if (e != hipSuccess) { if (tree) c->plan_serial = 0; return herr(e); }
    install.mark();
    return total_out ? read_total(c, total, total_out) : 0;
}

// what every scene query's kernels are handed: the scene's arrays, the n queries and their answers, the overflow word of the pass
SceneQuery scene_query(const bvh_scene* sc, const void* queries, uint32_t n, void* answers, uint32_t* overflow) {
    SceneQuery q;
    q.rays = queries; q.hits = answers; q.overflow = overflow;
    q.tnodes = sc->tnodes; q.tleaves = sc->tleaves; q.tparent = sc->tparent; q.inst = sc->inst; q.blas = sc->blas; q.wbox = sc->wbox;
    q.n_rays = n; q.n_inst = sc->n_inst; q.troot = sc->troot; q.tlayout = sc->tlayout; q.inst_in = sc->inst_in;
    return q;
}

// per-primitive algorithmic bytes of the whole pipeline (restated in DESIGN.md)
uint64_t algorithmic_bytes(bvh_algo a, uint32_t n) {
    static const uint64_t per_prim[4] = { 384, 420, 438, 386 };
    return per_prim[(int)a] * (uint64_t)n;
}

} // namespace

extern "C" {

const char* bvh_version(void) { return "bvh_mi355x 0.4 (gfx950)"; }
uint32_t bvh_abi_version(void) { return BVH_ABI_VERSION; }
void bvh_abi_struct_sizes(uint32_t out[3]) { if (out) { out[0] = (uint32_t)sizeof(bvh_result); out[1] = (uint32_t)sizeof(bvh_timings); out[2] = (uint32_t)sizeof(bvh_build_input); } }

int bvh_ctx_set_option(bvh_ctx* c, bvh_option option, int64_t value) {
    if (!c) return BVH_E_INVALID_ARG;
    switch (option) {
        case BVH_OPT_HPLOC_SCHEDULER: if (value < 0 || value > 3) return BVH_E_INVALID_ARG; if (value == 3) value = 2; break;   // (3: round 6's overlapped schedule, removed — same trees; still accepted, means 2)
        case BVH_OPT_LBVH_SCHEDULER: if (value < 0 || value > 2) return BVH_E_INVALID_ARG; break;
        case BVH_OPT_PLOC_SCHEDULER: if (value < 0 || value > 2) return BVH_E_INVALID_ARG; if (value == 2) value = 0; break;   // (2: ABI 4's cooperative launch, removed in round 5 — same trees; still accepted, means 0)
        case BVH_OPT_SORT_TEST_KNOBS: if (value & ~(int64_t)(8 | 32)) return BVH_E_INVALID_ARG; break;
        default: return BVH_E_INVALID_ARG;
    }
    c->options[(int)option] = value;
    c->sort.test_knobs = (int)c->options[BVH_OPT_SORT_TEST_KNOBS];
    c->ploc.static_ids = c->options[BVH_OPT_PLOC_SCHEDULER] == 0;
    return 0;
}
#ifdef BVH_ABLATION   // measurement build only: raw reads of the HPLOC queue buffers (the upper half of queue_rng doubles as a trace buffer: tools/ext_trace.py)
extern "C" int bvh_debug_read_queue(bvh_ctx* c, int which, size_t off_words, void* dst, size_t nwords) {
    if (!c || !dst) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return BVH_E_INTERNAL;
    if (which == 0) { if (hipMemcpy(dst, c->hploc.queue_count + off_words, nwords * 4, hipMemcpyDeviceToHost) != hipSuccess) return BVH_E_INTERNAL; }
    else if (which == 1) { if (off_words + nwords > c->hploc.queue_capacity || hipMemcpy(dst, c->hploc.queue_rng + off_words, nwords * 8, hipMemcpyDeviceToHost) != hipSuccess) return BVH_E_INTERNAL; }
    else if (which == 2) { *(uint64_t*)dst = c->hploc.queue_capacity; }
    else return BVH_E_INVALID_ARG;
    return 0;
}
#endif
int bvh_ctx_get_option(const bvh_ctx* c, bvh_option option, int64_t* value_out) {
#ifdef BVH_ABLATION   // measurement build only: option 1000 = merge tasks the HPLOC tile kernel ran in the last build (tools/measure_task_share.py)
    if (c && value_out && (int)option >= 1000 && (int)option < 1000 + 2046) {      // 1001..: the other measurement words of sub-queue 0's padded head (ABL_EXT_TIMING)
        u32 v = 0; Bind b(c->device);
        if (!c->hploc.queue_count || hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&v, c->hploc.queue_count + 2 + ((int)option - 1000), 4, hipMemcpyDeviceToHost) != hipSuccess) return BVH_E_INTERNAL;
        *value_out = v; return 0;
    }
#endif
    if (!c || !value_out || (int)option < 0 || (int)option > 3) return BVH_E_INVALID_ARG;
    *value_out = c->options[(int)option];
    return 0;
}

int bvh_ctx_create_on_stream(int device, void* hip_stream, bvh_ctx** out) {
    if (!out) return BVH_E_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return BVH_E_INVALID_ARG;
    Bind b(device); if (!b.ok) return BVH_E_INVALID_ARG;
    bvh_ctx* c = new (std::nothrow) bvh_ctx();
    if (!c) return BVH_E_INTERNAL;
    c->device = device;
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else { hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking); if (e != hipSuccess) { c->stream = nullptr; bvh_ctx_destroy(c); return -(int)e; } c->own_stream = true; }
    // (a failure from here on goes through bvh_ctx_destroy, which releases whatever exists: stream, events, pinned words)
    for (auto& e : c->ev) { hipError_t r = hipEventCreate(&e); if (r != hipSuccess) { e = nullptr; bvh_ctx_destroy(c); return -(int)r; } }
    { hipError_t r = hipHostMalloc(reinterpret_cast<void**>(&c->h_pinned), (16 + PLOC_STATE_WORDS) * sizeof(u32), hipHostMallocMapped); if (r != hipSuccess) { c->h_pinned = nullptr; bvh_ctx_destroy(c); return -(int)r; }
      void* dp = nullptr; r = hipHostGetDevicePointer(&dp, c->h_pinned, 0); if (r != hipSuccess) { bvh_ctx_destroy(c); return -(int)r; } c->d_pinned = static_cast<u32*>(dp); }
    // the build path's code objects are loaded here, once per process and device, not by a context's first build (first build of a fresh process at 262 144 triangles:
    // 2.4 ms against 0.13 warm; first HPLOC / PLOC++ build after that 0.51 / 0.65 against 0.18 / 0.38 — tools/cold_probe.py)
    { static std::once_flag warmed[64];
      std::call_once(warmed[device & 63], [] { warm_stage_em(); warm_sort(); warm_lbvh(); warm_hploc(); warm_ploc(); warm_misc(); warm_collapse(); warm_refit(); warm_refit_subset(); warm_query(); warm_optimize(); warm_scene(); warm_scene_point(); warm_scene_knn(); warm_scene_multihit(); warm_scene_radius(); warm_scene_overlap(); warm_scene_cull(); warm_scene_tris(); warm_scene_closest_tris(); warm_scene_radius_tris(); warm_scene_collide(); warm_scene_winding(); warm_point_query(); warm_winding(); warm_overlap(); warm_tris(); warm_closest_tris(); warm_knn(); warm_multihit(); warm_radius(); warm_radius_tris(); warm_split(); warm_many(); warm_many_ploc(); }); }
    *out = c;
    return 0;
}
int bvh_ctx_create(int device, bvh_ctx** out) { return bvh_ctx_create_on_stream(device, nullptr, out); }

void bvh_ctx_destroy(bvh_ctx* c) {
    if (!c) return;
    Bind b(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->arena) hipFree(c->arena);
    if (c->tris) hipFree(c->tris);
    if (c->subset_words) hipFree(c->subset_words);
    if (c->split_words) hipFree(c->split_words);
    if (c->many_items) hipFree(c->many_items);
    if (c->many_host) hipHostFree(c->many_host);
    if (c->many_ev) hipEventDestroy(c->many_ev);
    for (auto& e : c->ev) if (e) hipEventDestroy(e);
    if (c->h_pinned) hipHostFree(c->h_pinned);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int bvh_ctx_reserve(bvh_ctx* c, uint32_t n) { if (!c) return BVH_E_INVALID_ARG; Bind b(c->device); return ensure_capacity(c, n); }
int bvh_ctx_device(const bvh_ctx* c) { return c ? c->device : -1; }
void* bvh_ctx_stream(const bvh_ctx* c) { return c ? (void*)c->stream : nullptr; }
int bvh_ctx_set_profiling(bvh_ctx* c, int level) {
    if (!c) return BVH_E_INVALID_ARG;
    c->profiling = level != 0; c->kernel_profiling = level >= 2; c->recorder.reset(); c->build_counter = 0;   // (the next build is a sampled one)
    return 0;
}

// Sum of the per-kernel event times recorded since the last bvh_ctx_set_profiling(ctx, 2).  Synchronises the stream.
// names_out: buffer for '\n'-separated kernel names; ms_out/count_out: per distinct kernel (order of first launch).
int bvh_ctx_kernel_times(bvh_ctx* c, char* names_out, uint32_t names_cap, float* ms_out, uint32_t* count_out, uint32_t max_kernels) {
    if (!c) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<std::string> order; std::map<std::string, std::pair<double, uint32_t>> acc;
    for (size_t i = 0; i + 1 < c->recorder.used; ++i) {
        if (!c->recorder.recs[i].name) continue;              // end-of-build mark
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->recorder.recs[i].ev, c->recorder.recs[i + 1].ev));
        auto it = acc.find(c->recorder.recs[i].name);
        if (it == acc.end()) { order.push_back(c->recorder.recs[i].name); acc[c->recorder.recs[i].name] = {ms, 1u}; }
        else { it->second.first += ms; it->second.second += 1; }
    }
    std::string names; uint32_t k = 0;
    for (auto& nme : order) { if (k >= max_kernels) break; if (ms_out) ms_out[k] = (float)acc[nme].first; if (count_out) count_out[k] = acc[nme].second; names += nme; names += '\n'; ++k; }
    if (names_out && names_cap) { std::strncpy(names_out, names.c_str(), names_cap - 1); names_out[names_cap - 1] = 0; }
    return (int)k;
}
int bvh_ctx_last_collapse_ms(const bvh_ctx* c, float* ms_out) { if (!c || !ms_out) return BVH_E_INVALID_ARG; *ms_out = c->last_collapse_ms; return 0; }
int bvh_ctx_set_kernel_filter(bvh_ctx* c, const char* kernel_name) {
    if (!c) return BVH_E_INVALID_ARG;
    c->recorder.only = kernel_name ? kernel_name : ""; c->recorder.reset();
    return 0;
}
int bvh_ctx_set_kernel_sampling(bvh_ctx* c, uint32_t every) {
    if (!c || every == 0) return BVH_E_INVALID_ARG;
    c->sample_every = every; c->build_counter = 0; c->recorder.reset();
    return 0;
}
// the two overflow words of the ctx's last query call, after its work is done: how many queries the stack walks of the (count) pass and of the fill pass left
// to the stackless kernels.  Blocks on the stream and on an 8-byte read-back; for tests and diagnosis
int bvh_ctx_query_overflow(bvh_ctx* c, uint32_t* first_pass_out, uint32_t* fill_pass_out) {
    if (!c || !c->arena) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    u32 w[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(w, overflow_words(c), sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first_pass_out) *first_pass_out = w[0];
    if (fill_pass_out) *fill_pass_out = w[1];
    return 0;
}
int bvh_ctx_synchronize(bvh_ctx* c) { if (!c) return BVH_E_INVALID_ARG; Bind b(c->device); return herr(hipStreamSynchronize(c->stream)); }

int bvh_stage_extents(bvh_ctx* c, const void* d_tris, uint32_t n, void* d_prim_aabbs, void* d_scene_extent) {
    if (!c || !d_tris || !d_prim_aabbs || !d_scene_extent || n == 0) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    launch_extents(c->stream, d_tris, n, d_prim_aabbs, d_scene_extent);
    return herr(hipGetLastError());
}

int bvh_stage_morton(bvh_ctx* c, const void* d_prim_aabbs, uint32_t n, const void* d_scene_extent, uint32_t* d_keys, uint32_t* d_vals) {
    if (!c || !d_prim_aabbs || !d_scene_extent || !d_keys || n == 0) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    launch_morton(c->stream, d_prim_aabbs, n, d_scene_extent, d_keys, d_vals, nullptr, 0, 0);
    return herr(hipGetLastError());
}

int bvh_sort_pairs(bvh_ctx* c, const uint32_t* d_keys_in, const uint32_t* d_vals_in, uint32_t n, uint32_t* d_keys_out,
                   uint32_t* d_vals_out, int start_bit, int end_bit) {
    if (!c || !d_keys_in || !d_keys_out || !d_vals_out || n == 0 || start_bit < 0 || end_bit > 32 || start_bit > end_bit) return BVH_E_INVALID_ARG;
    if (n >= (1u << 30)) return BVH_E_TOO_LARGE;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    sort_prepare(c->stream, c->sort, n, sort_passes(start_bit, end_bit));
    sort_pairs(c->stream, c->sort, d_keys_in, d_vals_in, n, d_keys_out, d_vals_out, start_bit, end_bit, false);
    return herr(hipGetLastError());
}

int bvh_sort_pairs64(bvh_ctx* c, const uint64_t* d_keys_in, const uint32_t* d_vals_in, uint32_t n, uint64_t* d_keys_out,
                     uint32_t* d_vals_out, int start_bit, int end_bit) {
    if (!c || !d_keys_in || !d_keys_out || !d_vals_out || n == 0 || start_bit < 0 || end_bit > 64 || start_bit > end_bit) return BVH_E_INVALID_ARG;
    if (n >= (1u << 30)) return BVH_E_TOO_LARGE;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    sort_prepare(c->stream, c->sort, n, sort_passes(start_bit, end_bit));
    sort_pairs64(c->stream, c->sort, d_keys_in, d_vals_in, n, d_keys_out, d_vals_out, start_bit, end_bit, false);
    return herr(hipGetLastError());
}

int bvh_stage_morton64(bvh_ctx* c, const void* d_prim_aabbs, uint32_t n, const void* d_scene_extent, uint64_t* d_keys, int total_bits) {
    if (!c || !d_prim_aabbs || !d_scene_extent || !d_keys || n == 0 || total_bits < 3 || total_bits > 60) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    launch_morton64(c->stream, d_prim_aabbs, n, d_scene_extent, d_keys, total_bits, nullptr, 0);
    return herr(hipGetLastError());
}

int bvh_stage_morton_plan(bvh_ctx* c, const void* d_scene_extent, int total_bits, int32_t plan_out[10]) {
    if (!c || !d_scene_extent || !plan_out || total_bits < 3 || total_bits > 60) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, 2); if (r) return r;
    int* d = reinterpret_cast<int*>(c->small + 48);                      // 10 words of the ctx's small scratch
    launch_morton_plan(c->stream, d_scene_extent, d, total_bits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(plan_out, d, 10 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return herr(hipStreamSynchronize(c->stream));
}

int bvh_stage_extents_ex(bvh_ctx* c, const bvh_build_input* in, uint32_t n, void* d_prim_aabbs, void* d_scene_extent) {
    if (!c || !in || !d_prim_aabbs || !d_scene_extent || n == 0) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = stage_extents_fmt(c->stream, in, n, d_prim_aabbs, d_scene_extent); if (r) return r;
    return herr(hipGetLastError());
}

int bvh_emit_lbvh_single(bvh_ctx* c, const void* d_prim_aabbs, const uint32_t* d_sorted_keys, const uint32_t* d_sorted_vals,
                         uint32_t n, void* d_nodes, uint32_t* root_out) {
    if (!c || !d_prim_aabbs || !d_sorted_keys || !d_sorted_vals || !d_nodes || n < 2) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    ++c->tree_serial;
    r = begin_emit(c); if (r) return r;
    launch_lbvh_single(c->stream, d_prim_aabbs, d_sorted_keys, 32, d_sorted_vals, n, d_nodes, c->hploc.dep, c->small, c->ploc.list0, c->lbvh_queue_capacity, c->hploc.queue_count, false, (int)c->options[BVH_OPT_LBVH_SCHEDULER]);
    r = end_emit(c); if (r) return r;
    if (root_out) { r = read_back(c, c->small, 1, nullptr, 0, c->h_pinned); if (r) return r; *root_out = c->h_pinned[0]; }
    return 0;
}

int bvh_emit_lbvh_two(bvh_ctx* c, const void* d_prim_aabbs, const uint32_t* d_sorted_keys, const uint32_t* d_sorted_vals,
                      uint32_t n, void* d_nodes) {
    if (!c || !d_prim_aabbs || !d_sorted_keys || !d_sorted_vals || !d_nodes || n < 2) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    ++c->tree_serial;
    r = begin_emit(c); if (r) return r;
    launch_lbvh_two(c->stream, d_prim_aabbs, d_sorted_keys, 32, d_sorted_vals, n, d_nodes, c->parent, c->flags, c->hploc.dep, c->small,
                    c->ploc.list0, c->lbvh_queue_capacity, c->hploc.queue_count, false, (int)c->options[BVH_OPT_LBVH_SCHEDULER]);
    return end_emit(c);
}

int bvh_emit_ploc(bvh_ctx* c, const void* d_prim_aabbs, const uint32_t* d_sorted_vals, uint32_t n, void* d_nodes, void* d_leaves,
                  uint32_t* iterations_out) {
    if (!c || !d_prim_aabbs || !d_sorted_vals || !d_nodes || !d_leaves || n < 2) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    ++c->tree_serial;
    ploc_begin(c->stream, c->ploc, n);
    HIP_TRY(hipGetLastError());
    return run_ploc(c, n, d_nodes, d_leaves, d_prim_aabbs, d_sorted_vals, c->ploc, iterations_out);
}

int bvh_emit_hploc(bvh_ctx* c, const void* d_prim_aabbs, const uint32_t* d_sorted_keys, const uint32_t* d_sorted_vals, uint32_t n,
                   void* d_nodes, void* d_leaves) {
    if (!c || !d_prim_aabbs || !d_sorted_keys || !d_sorted_vals || !d_nodes || !d_leaves || n < 2) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    ++c->tree_serial;
    r = begin_emit(c); if (r) return r;
    emit_hploc(c, c->stream, d_prim_aabbs, d_sorted_keys, 32, d_sorted_vals, n, d_nodes, d_leaves);
    return end_emit(c);
}

#ifndef LEAF_FROM_TRIS
#define LEAF_FROM_TRIS 0
#endif
#ifndef SORT_GATE_TOP
#define SORT_GATE_TOP 1      // 0: the build sorts all 32 key bits at every size (no narrow top pass, no gate)
#endif
// d_in_boxes: bvh_build_boxes' input (bvh_aabb[n], device) — stage E copies those boxes instead of reading `in`'s triangles (in->morton_bits still applies)
static int build_impl(bvh_ctx* c, bvh_algo algo, const bvh_build_input* in, uint32_t n, bvh_result* out, bvh_timings* tm, const void* d_in_boxes = nullptr) {
    const int key_bits = in->morton_bits == 60 ? 64 : 32;
    hipStream_t s = c->stream;
    Install install(c);
    const bool prof = c->profiling && install.sampled;
    uint32_t ploc_iters = 0;
    int r = 0;
    ++c->tree_serial;                                         // (bvh_refit's cached parent plan no longer describes c->nodes)
    if (prof) HIP_TRY(hipEventRecord(c->ev[0], s));
    // E: CalculateSceneExtents (token CalculateCentroidExtentsTime).  The sort's bookkeeping is cleared here so that the
    // Morton kernel can accumulate the digit histograms.
    // the reference sorts all 32 key bits at its four call sites (src/Hploc.cpp:63-81 ...); the codes this build produces have 30 (60) significant bits, so
    // the build's own sort runs on bits [0, 30) / [0, 60): four (eight) passes either way, but the last one has a 6-bit (4-bit) digit — 64 digit threads,
    // 6 ballots per key and 64 status words per tile in the look-back instead of 256.  The fused digit histograms of the Morton kernel
    // — (code >> 24) & 255 for the last pass — hold exactly those digits' counts.  (bvh_sort_pairs keeps full generality for caller-supplied keys.)
    // Round 5: the reference's wrap-around code arithmetic leaves bits 30 / 31 (60..63) set on degenerate scenes (planar, axis ratio >= 2^32).  The u64 sort
    // therefore runs on all 64 bits (eight passes either way); the u32 sort keeps its 6-bit top pass but gates it on a device word the Morton kernel raises when
    // such a code exists — the full-width instantiation enqueued behind it then does the pass (SORT_WIDE_FLAG_WORD, kernels.hpp).
    // Same-box A/B of the gate (gpurun_out/r5_gate_ab.log): + 3 us per build (the second launch) against the 4.5 us the narrow pass saves at 10 M — and nothing to save
    // below the wide sort tiles' threshold (262 144: 0.1141 -> 0.1165 ms), where the build therefore simply sorts all 32 bits like the reference.
    const int end_bit = key_bits == 64 ? 64 : (n >= SORT_WIDE_MIN_N && SORT_GATE_TOP != 0) ? 30 : 32;
    const int passes = sort_passes(0, end_bit);
    if (!d_in_boxes) { r = stage_extents_valid(in); if (r) return r; }
    // what a build needs cleared (digit histograms, look-back status rows and tile tickets of `passes` sort passes, the emitters' queue heads) is cleared by
    // stage E's kernel itself; the scene extent of THIS build was reset by the previous build's Morton kernel (two extents, used alternately) — explicitly
    // only for a context's first build, after a re-allocation or after a build that failed half-way
    float* const scene = c->scene + 8 * c->scene_slot;
    float* const scene_next = c->scene + 8 * (c->scene_slot ^ 1);
    PrepArgs prep;
    prep.hist = c->sort.hist; prep.hist_words = (u32)SORT_HIST_COPIES * SORT_HIST_STRIDE;
    prep.status = reinterpret_cast<uint4*>(c->sort.status); prep.status_vecs = (u32)(((size_t)passes * sort_tiles(n) * SORT_RADIX) / 4);
    prep.counters = c->sort.counters; prep.extra = c->hploc.queue_count; prep.extra_words = hploc_head_words();
    if (algo == BVH_PLOCPP) ploc_begin_prep(c->ploc, n, prep);       // (the stage entry point bvh_emit_ploc launches k_ploc_init instead)
    const bool explicit_reset = !c->scene_ready;
    c->scene_ready = false;
    if (d_in_boxes) launch_extents_boxes(s, d_in_boxes, n, c->boxes, scene, explicit_reset, &prep);
    else { r = stage_extents_fmt(s, in, n, c->boxes, scene, explicit_reset, &prep); if (r) return r; }
    if (prof) HIP_TRY(hipEventRecord(c->ev[1], s));
    // M: CalculateMortonCodes (token CalculateMortonCodesTime); values are implicit (value i = i), produced by sort pass 0
    if (key_bits == 64) launch_morton64(s, c->boxes, n, scene, reinterpret_cast<u64*>(c->keys), 60, c->sort.hist, passes, scene_next);
    else launch_morton(s, c->boxes, n, scene, c->keys, nullptr, c->sort.hist, SORT_BITS, passes, scene_next);
    if (prof) HIP_TRY(hipEventRecord(c->ev[2], s));
    // S: radix sort (token SortingTime)
    if (key_bits == 64) sort_pairs64(s, c->sort, reinterpret_cast<const u64*>(c->keys), nullptr, n, reinterpret_cast<u64*>(c->skeys), c->svals, 0, end_bit, true);
    else sort_pairs(s, c->sort, c->keys, nullptr, n, c->skeys, c->svals, 0, end_bit, true, end_bit == 30);
    if (prof) HIP_TRY(hipEventRecord(c->ev[3], s));
    // B: hierarchy emit (token BvhBuildTime; SetupClusters is booked here, not under Morton as the reference does)
    out->d_leaves = nullptr; out->layout = 0; out->root = 0;
    r = begin_emit(c); if (r) return r;
    switch (algo) {
        case BVH_LBVH_SINGLEPASS: launch_lbvh_single(s, c->boxes, c->skeys, key_bits, c->svals, n, c->nodes, c->hploc.dep, c->small, c->ploc.list0, c->lbvh_queue_capacity, c->hploc.queue_count, true, (int)c->options[BVH_OPT_LBVH_SCHEDULER]); break;
        case BVH_LBVH_TWOPASS:    launch_lbvh_two(s, c->boxes, c->skeys, key_bits, c->svals, n, c->nodes, c->parent, c->flags, c->hploc.dep, c->small,
                                                  c->ploc.list0, c->lbvh_queue_capacity, c->hploc.queue_count, true, (int)c->options[BVH_OPT_LBVH_SCHEDULER]); break;
        case BVH_HPLOC:           c->hploc.leaf_tris = (LEAF_FROM_TRIS && !d_in_boxes && in->tri_format == BVH_TRI_PADDED64) ? in->d_tris : nullptr;
                                  emit_hploc(c, s, c->boxes, c->skeys, key_bits, c->svals, n, c->nodes, c->leaves, true);
                                  c->hploc.leaf_tris = nullptr;
                                  out->d_leaves = c->leaves; out->layout = 1; break;
        case BVH_PLOCPP:          r = run_ploc(c, n, c->nodes, c->leaves, c->boxes, c->svals, c->ploc, &ploc_iters); if (r) return r;
                                  out->d_leaves = c->leaves; out->layout = 1; break;
    }
    r = end_emit(c); if (r) return r;
    c->scene_ready = true; c->scene_slot ^= 1;             // every launch was accepted: the Morton kernel has reset the other extent for the next build
    install.mark();
    if (prof) HIP_TRY(hipEventRecord(c->ev[4], s));
    if (algo == BVH_LBVH_SINGLEPASS) {   // m_rootNodeIdx read-back (src/SinglePassLbvh.cpp:131)
        r = read_back(c, c->small, 1, nullptr, 0, c->h_pinned); if (r) return r;           // {root, ~root} into pinned words 0..1
        out->root = c->h_pinned[0];
        if (out->root >= 2u * n - 1u) return BVH_E_INTERNAL;                               // (an index that consumers turn into an address)
    }
    out->d_nodes = c->nodes; out->d_prim_aabbs = c->boxes; out->d_scene_extent = scene;
    out->d_sorted_keys = c->skeys; out->d_sorted_vals = c->svals;
    out->n_internal = n - 1; out->n_leaves = n; out->key_bits = (uint32_t)key_bits; out->reserved = 0;
    out->d_tris = d_in_boxes ? nullptr : in->tri_format == BVH_TRI_INDEXED ? in->d_vertices : in->d_tris; out->d_morton_keys = c->keys;
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->bytes_algorithmic = algorithmic_bytes(algo, n);
        tm->ploc_iterations = ploc_iters;
        tm->sampled = prof ? 1u : 0u;
        if (prof) {
            HIP_TRY(hipEventSynchronize(c->ev[4]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_extents, c->ev[0], c->ev[1]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_morton, c->ev[1], c->ev[2]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_sort, c->ev[2], c->ev[3]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_build, c->ev[3], c->ev[4]));
            tm->ms_total = tm->ms_extents + tm->ms_morton + tm->ms_sort + tm->ms_build;
        }
    }
    return 0;
}

int bvh_build(bvh_ctx* c, bvh_algo algo, const void* tris, uint32_t n, int tris_on_device, bvh_result* out, bvh_timings* tm) {
    if (!c || !tris || !out || n < 2 || (int)algo < 0 || (int)algo > 3) return BVH_E_INVALID_ARG;
    if (n >= (1u << 30)) return BVH_E_TOO_LARGE;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    bvh_build_input in; std::memset(&in, 0, sizeof in);
    in.tri_format = BVH_TRI_PADDED64; in.morton_bits = 30; in.d_tris = tris;
    if (!tris_on_device) {   // H2D copy of the input, outside the timers (src/TwoPassLbvh.cpp:19-20)
        r = ensure_tris(c, n); if (r) return r;
        HIP_TRY(hipMemcpyAsync(c->tris, tris, (size_t)n * sizeof(bvh_triangle), hipMemcpyHostToDevice, c->stream));
        in.d_tris = c->tris;
    }
    return build_impl(c, algo, &in, n, out, tm);
}

int bvh_build_ex(bvh_ctx* c, bvh_algo algo, const bvh_build_input* in, uint32_t n, bvh_result* out, bvh_timings* tm) {
    if (!c || !in || !out || n < 2 || (int)algo < 0 || (int)algo > 3) return BVH_E_INVALID_ARG;
    if (in->morton_bits != 30 && in->morton_bits != 60) return BVH_E_INVALID_ARG;
    if (n >= (1u << 30)) return BVH_E_TOO_LARGE;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    return build_impl(c, algo, in, n, out, tm);
}

int bvh_build_boxes(bvh_ctx* c, bvh_algo algo, const void* d_boxes, uint32_t n, int morton_bits, bvh_result* out, bvh_timings* tm) {
    if (!c || !d_boxes || !out || n < 2 || (int)algo < 0 || (int)algo > 3) return BVH_E_INVALID_ARG;
    if (morton_bits != 30 && morton_bits != 60) return BVH_E_INVALID_ARG;
    if (n >= (1u << 30)) return BVH_E_TOO_LARGE;
    Bind b(c->device);
    int r = ensure_capacity(c, n); if (r) return r;
    bvh_build_input in; std::memset(&in, 0, sizeof in);
    in.tri_format = BVH_TRI_PADDED64; in.morton_bits = (uint32_t)morton_bits;
    return build_impl(c, algo, &in, n, out, tm, d_boxes);
}

// ---- refit (no counterpart in the reference) ----------------------------------------------------------------------------------------------------
// what bvh_refit may touch is checked before anything is enqueued: an error changes nothing.  The arena is never re-allocated (io may point into it).
static int refit_check(const bvh_ctx* c, const bvh_result* io) {
    if (!c || !io) return BVH_E_INVALID_ARG;
    if (!tree_valid(io) || !io->d_prim_aabbs || !io->d_scene_extent) return BVH_E_INVALID_ARG;
    if (io->n_leaves > c->cap) return BVH_E_INVALID_ARG;      // (parent / flags scratch is sized by the capacity: bvh_ctx_reserve first)
    return 0;
}
// stage E into io's prim boxes and scene extent (the result's own extent slot: the other slot and the ctx's scene bookkeeping are untouched), the parent plan
// unless the ctx's own tree has one, the refit climb.  Timings: ms_extents = stage E, ms_build = plan + climb (bvh_ctx_kernel_times names them apart)
static int refit_impl(bvh_ctx* c, bvh_result* io, const bvh_build_input* in, bvh_timings* tm) {
    hipStream_t s = c->stream;
    const uint32_t n = io->n_leaves;
    Install install(c);
    const bool prof = c->profiling && install.sampled;
    if (prof) HIP_TRY(hipEventRecord(c->ev[0], s));
    int r = stage_extents_fmt(s, in, n, io->d_prim_aabbs, io->d_scene_extent, true, nullptr); if (r) return r;
    if (prof) HIP_TRY(hipEventRecord(c->ev[1], s));
    r = begin_emit(c); if (r) return r;
    const bool own = io->d_nodes == c->nodes;
    if (!own || c->plan_serial != c->tree_serial || c->plan_n != n || c->plan_root != io->root) {
        launch_refit_plan(s, io->d_nodes, n, io->root, c->parent);
        c->plan_serial = own ? c->tree_serial : 0; c->plan_n = n; c->plan_root = io->root;
    }
    launch_refit_climb(s, io->d_prim_aabbs, io->d_nodes, io->d_leaves, (int)io->layout, n, c->parent, c->flags);
    r = end_emit(c); if (r) { c->plan_serial = 0; return r; }
    install.mark();
    if (prof) HIP_TRY(hipEventRecord(c->ev[4], s));
    io->d_tris = in->tri_format == BVH_TRI_INDEXED ? in->d_vertices : in->d_tris;
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->bytes_algorithmic = 200ull * n;          // nominal, 64-byte triangles (DESIGN.md "Refit")
        tm->sampled = prof ? 1u : 0u;
        if (prof) {
            HIP_TRY(hipEventSynchronize(c->ev[4]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_extents, c->ev[0], c->ev[1]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_build, c->ev[1], c->ev[4]));
            tm->ms_total = tm->ms_extents + tm->ms_build;
        }
    }
    return 0;
}

int bvh_refit(bvh_ctx* c, bvh_result* io, const void* tris, int tris_on_device, bvh_timings* tm) {
    int r = refit_check(c, io); if (r) return r;
    if (!tris) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    bvh_build_input in; std::memset(&in, 0, sizeof in);
    in.tri_format = BVH_TRI_PADDED64; in.morton_bits = 30; in.d_tris = tris;
    if (!tris_on_device) {   // H2D copy into the ctx's staging buffer (not part of the arena), untimed as for a build
        r = ensure_tris(c, io->n_leaves); if (r) return r;
        HIP_TRY(hipMemcpyAsync(c->tris, tris, (size_t)io->n_leaves * sizeof(bvh_triangle), hipMemcpyHostToDevice, c->stream));
        in.d_tris = c->tris;
    }
    return refit_impl(c, io, &in, tm);
}

int bvh_refit_ex(bvh_ctx* c, bvh_result* io, const bvh_build_input* in, bvh_timings* tm) {
    int r = refit_check(c, io); if (r) return r;
    if (!in) return BVH_E_INVALID_ARG;
    r = stage_extents_valid(in); if (r) return r;
    Bind b(c->device);
    return refit_impl(c, io, in, tm);
}

// ---- partial refit (no counterpart in the reference) --------------------------------------------------------------------------------------------
// the words of bvh_refit_subset, sized by the ctx's capacity.  The new block is allocated before the old one is released: a failed allocation changes nothing
static int ensure_subset_words(bvh_ctx* c) {
    if (c->subset_words && c->subset_cap == c->cap) return 0;
    u32* p = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), (size_t)c->cap * 3 * sizeof(u32)));
    if (c->subset_words) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipFree(c->subset_words);
        if (e != hipSuccess) { (void)hipFree(p); return -(int)e; }
    }
    c->subset_words = p; c->subset_cap = c->cap; c->map_serial = 0;
    c->subset_dirty = true;                                   // (zeroed by the call that follows, on the ctx's stream)
    return 0;
}

// Checked before anything is enqueued: an error changes nothing.  Then: the parent plan and the leaf map unless the ctx's own tree has them, the box pass over the
// list, mark + climb.  Timings: ms_extents = the box pass, ms_build = plan + map + mark + climb (bvh_ctx_kernel_times names them apart)
int bvh_refit_subset(bvh_ctx* c, bvh_result* io, const bvh_build_input* in, const uint32_t* d_prims, uint32_t n_dirty, bvh_timings* tm) {
    int r = refit_check(c, io); if (r) return r;
    bvh_build_input inp; std::memset(&inp, 0, sizeof inp);
    if (in) { r = stage_extents_valid(in); if (r) return r; inp = *in; }
    else { if (!io->d_tris) return BVH_E_INVALID_ARG; inp.tri_format = BVH_TRI_PADDED64; inp.d_tris = io->d_tris; }
    if ((n_dirty && !d_prims) || n_dirty >= (1u << 30)) return BVH_E_INVALID_ARG;
    const uint32_t n = io->n_leaves;
    {   // the list may not overlap what the call writes
        Range w[6] = { Range(io->d_prim_aabbs, (uint64_t)n * sizeof(bvh_aabb)), Range(io->d_scene_extent, sizeof(bvh_aabb)),
                       Range(c->parent, (uint64_t)c->cap * 2 * sizeof(u32)), Range(c->subset_words, (uint64_t)c->subset_cap * 3 * sizeof(u32)) };
        const int k = 4 + tree_ranges(io, w + 4);
        if (crosses(Range(d_prims, (uint64_t)n_dirty * sizeof(u32)), w, k)) return BVH_E_INVALID_ARG;
    }
    if (n_dirty == 0) return 0;
    Bind b(c->device);
    r = ensure_subset_words(c); if (r) return r;
    hipStream_t s = c->stream;
    u32* const leaf_of_prim = c->subset_words; u32* const owner = leaf_of_prim + c->subset_cap; u32* const pending = owner + c->subset_cap;
    Install install(c);
    const bool prof = c->profiling && install.sampled;
    const bool own = io->d_nodes == c->nodes;
    // caller-owned arrays may be anything: arrays that are not a tree can leave marks behind, so the call after one of theirs starts from zeroed words
    if (c->subset_dirty) HIP_TRY(hipMemsetAsync(owner, 0, (size_t)c->subset_cap * 2 * sizeof(u32), s));
    c->subset_dirty = true;
    if (prof) HIP_TRY(hipEventRecord(c->ev[0], s));
    if (!own || c->plan_serial != c->tree_serial || c->plan_n != n || c->plan_root != io->root) {
        launch_refit_plan(s, io->d_nodes, n, io->root, c->parent);
        c->plan_serial = own ? c->tree_serial : 0; c->plan_n = n; c->plan_root = io->root;
    }
    if (!own || c->map_serial != c->tree_serial || c->map_n != n || c->map_root != io->root) {
        launch_refit_leafmap(s, io->d_nodes, io->d_leaves, (int)io->layout, n, leaf_of_prim);
        c->map_serial = own ? c->tree_serial : 0; c->map_n = n; c->map_root = io->root;
    }
    if (prof) HIP_TRY(hipEventRecord(c->ev[1], s));
    launch_refit_subset_boxes(s, (int)inp.tri_format, inp.d_tris, inp.d_vertices, inp.d_indices, inp.n_vertices, d_prims, n_dirty, leaf_of_prim, owner,
                              io->d_prim_aabbs, io->d_nodes, io->d_leaves, (int)io->layout, n);
    if (prof) HIP_TRY(hipEventRecord(c->ev[2], s));
    launch_refit_subset_climb(s, d_prims, n_dirty, leaf_of_prim, owner, pending, c->parent, io->d_prim_aabbs, io->d_nodes, io->d_leaves, (int)io->layout, n, io->root,
                              io->d_scene_extent);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { c->plan_serial = 0; c->map_serial = 0; return -(int)e; } }
    c->subset_dirty = !own;                                   // (marks that caller-owned arrays left behind never reach the next call, whoever's tree it is on)
    install.mark();
    if (prof) HIP_TRY(hipEventRecord(c->ev[4], s));
    io->d_tris = inp.tri_format == BVH_TRI_INDEXED ? inp.d_vertices : inp.d_tris;
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->sampled = prof ? 1u : 0u;
        if (prof) {
            float ms_plan = 0.f, ms_climb = 0.f;
            HIP_TRY(hipEventSynchronize(c->ev[4]));
            HIP_TRY(hipEventElapsedTime(&ms_plan, c->ev[0], c->ev[1]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_extents, c->ev[1], c->ev[2]));
            HIP_TRY(hipEventElapsedTime(&ms_climb, c->ev[2], c->ev[4]));
            tm->ms_build = ms_plan + ms_climb;
            tm->ms_total = tm->ms_extents + tm->ms_build;
        }
    }
    return 0;
}

// ---- ray queries (no counterpart in the reference) ----------------------------------------------------------------------------------------------
// the checks bvh_intersect and bvh_closest_point share: every argument is checked before anything is enqueued, so an error writes nothing.  The arena is never
// re-allocated (the tree may point into it).  in = the validated triangles; d_q / d_h: the query and answer arrays (q_bytes / h_bytes long), which must not overlap
static int query_check(const bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, int query, const void* d_q, uint64_t q_bytes, const void* d_h,
                       uint64_t h_bytes, bvh_build_input* in) {
    if (!c || !tree || !d_q || !d_h) return BVH_E_INVALID_ARG;
    if (!tree_valid(tree) || resolve_tris(tree, tris, in)) return BVH_E_INVALID_ARG;
    if (query != BVH_QUERY_CLOSEST && query != BVH_QUERY_ANY) return BVH_E_INVALID_ARG;
    if (crosses(Range(d_q, q_bytes), Range(d_h, h_bytes))) return BVH_E_INVALID_ARG;
    if (tree->n_leaves > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    return 0;
}

int bvh_intersect(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_ray* d_rays, uint32_t n_rays, bvh_hit* d_hits, int query) {
    bvh_build_input in;
    int r = query_check(c, tree, tris, query, d_rays, (uint64_t)n_rays * sizeof(bvh_ray), d_hits, (uint64_t)n_rays * sizeof(bvh_hit), &in); if (r) return r;
    if (n_rays == 0) return 0;
    return query_tail(c, tree, overflow_words(c), [&](hipStream_t s, u32* overflow) {
        launch_intersect(s, (int)tree->layout, query, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_rays, n_rays, tree->d_nodes, tree->d_leaves,
                         tree->n_leaves, tree->root, d_hits, overflow, c->parent);
    });
}

// ---- point queries (no counterpart in the reference) ----------------------------------------------------------------------------------------------
// bvh_intersect's checks and tail
int bvh_closest_point(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_point_query* d_points, uint32_t n_points, bvh_point_hit* d_hits,
                      int query) {
    bvh_build_input in;
    int r = query_check(c, tree, tris, query, d_points, (uint64_t)n_points * sizeof(bvh_point_query), d_hits, (uint64_t)n_points * sizeof(bvh_point_hit), &in);
    if (r) return r;
    if (n_points == 0) return 0;
    return query_tail(c, tree, overflow_words(c), [&](hipStream_t s, u32* overflow) {
        launch_closest_point(s, (int)tree->layout, query, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_points, n_points,
                             tree->d_nodes, tree->d_leaves, tree->n_leaves, tree->root, d_hits, overflow, c->parent);
    });
}

// ---- winding numbers (no counterpart in the reference) ----------------------------------------------------------------------------------------------
// the tree / triangle checks of query_check and the moments array's own; every argument is checked before anything is enqueued, so an error writes nothing.
// rg / n_rg: the byte ranges of the tree's and the triangles' arrays and, last, of d_moments, which may overlap none of them
static int winding_check(const bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const void* d_moments, bvh_build_input* in, Range* rg, int* n_rg) {
    if (!c || !tree || !d_moments || ((uintptr_t)d_moments & 15u)) return BVH_E_INVALID_ARG;
    if (!tree_valid(tree) || resolve_tris(tree, tris, in)) return BVH_E_INVALID_ARG;
    if (tree->n_leaves > c->cap) return BVH_E_INVALID_ARG;    // (the parent plan and the exchange words live in the arena: bvh_ctx_reserve first)
    int k = tree_ranges(tree, rg);
    k += mesh_ranges(*in, tree->n_leaves, rg + k);
    rg[k] = Range(d_moments, (uint64_t)(tree->n_leaves - 1) * sizeof(bvh_winding_moment));
    *n_rg = k + 1;
    return crosses(rg[k], rg, k) ? BVH_E_INVALID_ARG : 0;
}

// bvh_refit's plan (cached under its rule), then the climb on the self-cleaning flags words (begin_emit / end_emit as for a refit) and the finalise
int bvh_winding_prepare(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, bvh_winding_moment* d_moments) {
    bvh_build_input in; Range rg[5]; int n_rg = 0;
    int r = winding_check(c, tree, tris, d_moments, &in, rg, &n_rg); if (r) return r;
    Bind b(c->device);
    hipStream_t s = c->stream;
    Install install(c);
    r = begin_emit(c); if (r) return r;
    query_plan(c, tree, s);
    launch_winding_prepare(s, (int)tree->layout, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, tree->d_nodes, tree->d_leaves,
                           tree->n_leaves, c->parent, c->flags, d_moments);
    r = end_emit(c); if (r) { c->plan_serial = 0; return r; }
    install.mark();
    return 0;
}

// bvh_closest_point's tail
int bvh_winding_number(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_winding_moment* d_moments, const bvh_point_query* d_points,
                       uint32_t n_points, float beta, float* d_w) {
    bvh_build_input in; Range rg[6]; int n_rg = 0;
    int r = winding_check(c, tree, tris, d_moments, &in, rg, &n_rg); if (r) return r;
    if (!d_points || !d_w || !(beta >= 0.0f)) return BVH_E_INVALID_ARG;     // (a NaN beta fails the comparison)
    rg[n_rg] = Range(d_points, (uint64_t)n_points * sizeof(bvh_point_query));
    if (crosses(rg[n_rg], rg[n_rg - 1])) return BVH_E_INVALID_ARG;          // the points against the moments; the answers against everything
    if (crosses(Range(d_w, (uint64_t)n_points * sizeof(float)), rg, n_rg + 1)) return BVH_E_INVALID_ARG;
    if (n_points == 0) return 0;
    return query_tail(c, tree, overflow_words(c), [&](hipStream_t s, u32* overflow) {
        launch_winding(s, (int)tree->layout, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_points, n_points, tree->d_nodes,
                       tree->d_leaves, tree->n_leaves, tree->root, d_moments, beta, d_w, overflow, c->parent);
    });
}

// ---- k-nearest queries (no counterpart in the reference) -------------------------------------------------------------------------------------------
// bvh_closest_point's checks (query_check with the lists as the answer array) plus k's range, the list array's size and the third range; then its tail
int bvh_knn(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_point_query* d_points, uint32_t n_points, uint32_t k, bvh_knn_hit* d_hits,
            uint32_t* d_counts) {
    if (k == 0u || k > (uint32_t)BVH_KNN_MAX_K) return BVH_E_INVALID_ARG;
    const uint64_t p_bytes = (uint64_t)n_points * sizeof(bvh_point_query), h_bytes = (uint64_t)n_points * k * sizeof(bvh_knn_hit);
    if ((uint64_t)n_points * k >= (1ull << 32)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    int r = query_check(c, tree, tris, BVH_QUERY_CLOSEST, d_points, p_bytes, d_hits, h_bytes, &in);
    if (r) return r;
    const Range ph[2] = { Range(d_points, p_bytes), Range(d_hits, h_bytes) };
    if (crosses(Range(d_counts, (uint64_t)n_points * sizeof(u32)), ph, 2)) return BVH_E_INVALID_ARG;     // the third range: against the points and against the lists
    if (n_points == 0) return 0;
    return query_tail(c, tree, overflow_words(c), [&](hipStream_t s, u32* overflow) {
        launch_knn(s, (int)tree->layout, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_points, n_points, k, tree->d_nodes,
                   tree->d_leaves, tree->n_leaves, tree->root, d_hits, d_counts, overflow, c->parent);
    });
}

// ---- box queries (no counterpart in the reference) ------------------------------------------------------------------------------------------------
// count -> scan -> fill on one stream (count_fill_tail); every argument is checked before anything is enqueued, so an error writes nothing.  The arena is never
// re-allocated (the tree may point into it).  Whether the fill runs is decided on the device (overlap.hip); the host only waits when the caller asks for the total.
int bvh_overlap(bvh_ctx* c, const bvh_result* tree, const bvh_aabb* d_boxes, uint32_t n_boxes, int mode, uint32_t* d_offsets, uint32_t* d_prims,
                uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_boxes || !d_offsets) return BVH_E_INVALID_ARG;
    if (!tree_valid(tree)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (mode != BVH_OVERLAP_BOXES && mode != BVH_OVERLAP_SELF) return BVH_E_INVALID_ARG;
    if (mode == BVH_OVERLAP_SELF && n_boxes != n) return BVH_E_INVALID_ARG;
    if (n_boxes >= (1u << 30)) return BVH_E_INVALID_ARG;
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    const Range rs[3] = { Range(d_boxes, (uint64_t)n_boxes * sizeof(bvh_aabb)), Range(d_offsets, ((uint64_t)n_boxes + 1u) * sizeof(u32)),
                          fill_range(d_prims, capacity, sizeof(u32)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(c, tree, n_boxes, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_overlap_count(s, (int)tree->layout, mode, d_boxes, n_boxes, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, overflow, c->parent,
                             c->overlap_sums, total);
        if (d_prims)
            launch_overlap_fill(s, (int)tree->layout, mode, d_boxes, n_boxes, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_prims, capacity, total,
                                overflow + 1, c->parent);
    });
}

// ---- convex-volume queries (no counterpart in the reference) ---------------------------------------------------------------------------------------
// bvh_overlap's checks and tail, with planes in place of boxes; every argument is checked before anything is enqueued, so an error writes nothing.  The walk is
// chosen here: BVH_CULL_AUTO takes the group walk for few volumes on a tree large enough to fill a workgroup's rounds (kernels.hpp's two constants)
int bvh_cull(bvh_ctx* c, const bvh_result* tree, const float* d_planes, uint32_t n_volumes, uint32_t planes_per_volume, int path, uint32_t* d_offsets,
             bvh_cull_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_planes || !d_offsets) return BVH_E_INVALID_ARG;
    if (!tree_valid(tree)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (planes_per_volume < 1u || planes_per_volume > (uint32_t)BVH_CULL_MAX_PLANES) return BVH_E_INVALID_ARG;
    if (path != BVH_CULL_AUTO && path != BVH_CULL_LANE && path != BVH_CULL_GROUP) return BVH_E_INVALID_ARG;
    if (n_volumes >= (1u << 30)) return BVH_E_INVALID_ARG;
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    const Range rs[3] = { Range(d_planes, (uint64_t)n_volumes * planes_per_volume * 4u * sizeof(float)), Range(d_offsets, ((uint64_t)n_volumes + 1u) * sizeof(u32)),
                          fill_range(d_hits, capacity, sizeof(bvh_cull_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    const bool group = path == BVH_CULL_GROUP || (path == BVH_CULL_AUTO && n_volumes <= CULL_AUTO_MAX_VOLUMES && n >= CULL_AUTO_MIN_LEAVES);
    return count_fill_tail(c, tree, n_volumes, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_cull_count(s, (int)tree->layout, group, d_planes, n_volumes, planes_per_volume, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, overflow,
                          c->parent, c->overlap_sums, total);
        if (d_hits)
            launch_cull_fill(s, (int)tree->layout, group, d_planes, n_volumes, planes_per_volume, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_hits,
                             capacity, total, overflow + 1, c->parent);
    });
}

// ---- crossing triangle pairs (no counterpart in the reference) -------------------------------------------------------------------------------------
// bvh_overlap's tail, with the query mesh's triangles in place of boxes; every argument is checked before anything is enqueued, so an error writes nothing.
// Neither output array may overlap the other or any array the call reads
int bvh_intersect_tris(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_build_input* queries, uint32_t n_queries, int mode,
                       uint32_t* d_offsets, uint32_t* d_prims, uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_offsets) return BVH_E_INVALID_ARG;
    if (mode != BVH_TRIS_QUERY && mode != BVH_TRIS_SELF) return BVH_E_INVALID_ARG;
    if ((mode == BVH_TRIS_SELF) != (queries == nullptr)) return BVH_E_INVALID_ARG;       // the other mesh, or none in self mode
    if (!tree_valid(tree)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (mode == BVH_TRIS_SELF && n_queries != n) return BVH_E_INVALID_ARG;
    if (n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    if (resolve_tris(tree, tris, &in)) return BVH_E_INVALID_ARG;
    bvh_build_input qin = in;                                 // (self mode: the tree's own triangles)
    if (queries) { if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG; qin = *queries; }
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    {   // the output arrays against each other and against everything the call reads
        Range rs[8] = { Range(d_offsets, ((uint64_t)n_queries + 1u) * sizeof(u32)), fill_range(d_prims, capacity, sizeof(u32)) };
        int k = 2 + tree_ranges(tree, rs + 2);
        k += mesh_ranges(in, n, rs + k);
        if (queries) k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 2, k)) return BVH_E_INVALID_ARG;
    }
    const TrisMesh tm{ (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices };
    const TrisMesh qm{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices };
    return count_fill_tail(c, tree, n_queries, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_tris_count(s, (int)tree->layout, mode, tm, qm, n_queries, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, overflow, c->parent,
                          c->overlap_sums, total);
        if (d_prims)
            launch_tris_fill(s, (int)tree->layout, mode, tm, qm, n_queries, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_prims, capacity, total,
                             overflow + 1, c->parent);
    });
}

// ---- mesh-to-mesh distance (no counterpart in the reference) --------------------------------------------------------------------------------------
// bvh_closest_point's checks (query_check: the hit array stands in for the query array, whose ranges are checked below) and tail, bvh_intersect_tris's
// validation of the query mesh; every argument is checked before anything is enqueued, so an error writes nothing.  d_hits may overlap no array the call reads
int bvh_closest_tris(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_build_input* queries, uint32_t n_queries, float radius,
                     bvh_tri_hit* d_hits, int query) {
    if (!queries || n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    int r = query_check(c, tree, tris, query, d_hits, 0, d_hits, 0, &in); if (r) return r;
    if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG;
    const bvh_build_input qin = *queries;
    {   // the answers against everything the call reads
        Range rs[7] = { Range(d_hits, (uint64_t)n_queries * sizeof(bvh_tri_hit)) };
        int k = 1 + tree_ranges(tree, rs + 1);
        k += mesh_ranges(in, tree->n_leaves, rs + k);
        k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 1, k)) return BVH_E_INVALID_ARG;
    }
    if (n_queries == 0) return 0;
    const TrisMesh tm{ (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices };
    const TrisMesh qm{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices };
    return query_tail(c, tree, overflow_words(c), [&](hipStream_t s, u32* overflow) {
        launch_closest_tris(s, (int)tree->layout, query, tm, qm, n_queries, radius, tree->d_nodes, tree->d_leaves, tree->n_leaves, tree->root, d_hits, overflow,
                            c->parent);
    });
}

// ---- every triangle within a radius, mesh to mesh (no counterpart in the reference) ---------------------------------------------------------------
// bvh_intersect_tris's checks (its self-mode rules on the flag bits, its ranges with bvh_tri_hit records in place of words) and bvh_radius_search's tail;
// every argument is checked before anything is enqueued, so an error writes nothing
int bvh_radius_tris(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_build_input* queries, uint32_t n_queries, float radius,
                    uint32_t flags, uint32_t* d_offsets, bvh_tri_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_offsets) return BVH_E_INVALID_ARG;
    if (flags & ~(BVH_RADIUS_TRIS_SORTED | BVH_RADIUS_TRIS_SELF | BVH_RADIUS_TRIS_SKIP_SHARED)) return BVH_E_INVALID_ARG;
    const bool self = (flags & BVH_RADIUS_TRIS_SELF) != 0u;
    if ((flags & BVH_RADIUS_TRIS_SKIP_SHARED) && !self) return BVH_E_INVALID_ARG;
    if (self != (queries == nullptr)) return BVH_E_INVALID_ARG;                          // the other mesh, or none in self mode
    if (!tree_valid(tree)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (self && n_queries != n) return BVH_E_INVALID_ARG;
    if (n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    if (resolve_tris(tree, tris, &in)) return BVH_E_INVALID_ARG;
    bvh_build_input qin = in;                                 // (self mode: the tree's own triangles)
    if (queries) { if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG; qin = *queries; }
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    {   // the output arrays against each other and against everything the call reads
        Range rs[8] = { Range(d_offsets, ((uint64_t)n_queries + 1u) * sizeof(u32)), fill_range(d_hits, capacity, sizeof(bvh_tri_hit)) };
        int k = 2 + tree_ranges(tree, rs + 2);
        k += mesh_ranges(in, n, rs + k);
        if (queries) k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 2, k)) return BVH_E_INVALID_ARG;
    }
    const TrisMesh tm{ (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices };
    const TrisMesh qm{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices };
    return count_fill_tail(c, tree, n_queries, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_radius_tris_count(s, (int)tree->layout, flags, tm, qm, n_queries, radius, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, overflow, c->parent,
                                 c->overlap_sums, total);
        if (d_hits)
            launch_radius_tris_fill(s, (int)tree->layout, flags, tm, qm, n_queries, radius, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_hits, capacity,
                                    total, overflow + 1, c->parent);
    });
}

// ---- all-hits ray queries (no counterpart in the reference) ---------------------------------------------------------------------------------------
// bvh_intersect's tree / triangle checks and bvh_overlap's tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_intersect_all(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_ray* d_rays, uint32_t n_rays, uint32_t flags,
                      uint32_t* d_offsets, bvh_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_rays || !d_offsets) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_HITS_SORTED) return BVH_E_INVALID_ARG;
    if (n_rays >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    if (!tree_valid(tree) || resolve_tris(tree, tris, &in)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    const Range rs[3] = { Range(d_rays, (uint64_t)n_rays * sizeof(bvh_ray)), Range(d_offsets, ((uint64_t)n_rays + 1u) * sizeof(u32)),
                          fill_range(d_hits, capacity, sizeof(bvh_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(c, tree, n_rays, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_hits_count(s, (int)tree->layout, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_rays, n_rays, tree->d_nodes,
                          tree->d_leaves, n, tree->root, d_offsets, overflow, c->parent, c->overlap_sums, total);
        if (d_hits)
            launch_hits_fill(s, (int)tree->layout, (int)in.tri_format, (flags & BVH_HITS_SORTED) ? 1 : 0, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices,
                             d_rays, n_rays, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_hits, capacity, total, overflow + 1, c->parent);
    });
}

// ---- radius searches (no counterpart in the reference) -------------------------------------------------------------------------------------------
// bvh_closest_point's tree / triangle checks and bvh_intersect_all's tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_radius_search(bvh_ctx* c, const bvh_result* tree, const bvh_build_input* tris, const bvh_point_query* d_points, uint32_t n_points, uint32_t flags,
                      uint32_t* d_offsets, bvh_knn_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!c || !tree || !d_points || !d_offsets) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_RADIUS_SORTED) return BVH_E_INVALID_ARG;
    if (n_points >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input in;
    if (!tree_valid(tree) || resolve_tris(tree, tris, &in)) return BVH_E_INVALID_ARG;
    const uint32_t n = tree->n_leaves;
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (the parent plan lives in the arena's parent array: bvh_ctx_reserve first)
    const Range rs[3] = { Range(d_points, (uint64_t)n_points * sizeof(bvh_point_query)), Range(d_offsets, ((uint64_t)n_points + 1u) * sizeof(u32)),
                          fill_range(d_hits, capacity, sizeof(bvh_knn_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(c, tree, n_points, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        launch_radius_count(s, (int)tree->layout, (int)in.tri_format, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices, d_points, n_points, tree->d_nodes,
                            tree->d_leaves, n, tree->root, d_offsets, overflow, c->parent, c->overlap_sums, total);
        if (d_hits)
            launch_radius_fill(s, (int)tree->layout, (int)in.tri_format, (flags & BVH_RADIUS_SORTED) ? 1 : 0, in.d_tris, in.d_vertices, in.d_indices, in.n_vertices,
                               d_points, n_points, tree->d_nodes, tree->d_leaves, n, tree->root, d_offsets, d_hits, capacity, total, overflow + 1, c->parent);
    });
}

// ---- early split clipping (Utility::doEarlySplitClipping, src/Utility.cpp:456-538, as a device pass) ----------------------------------------------
// bvh_split_refs' words, sized by the largest n seen.  The new block is allocated before the old one is released: a failed allocation changes nothing
static constexpr size_t SPLIT_HEAD_BYTES = 64 + (size_t)OVERLAP_SCAN_BLOCKS * sizeof(u64);
static int ensure_split_words(bvh_ctx* c, uint32_t n) {
    if (c->split_words && n <= c->split_cap) return 0;
    char* p = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), SPLIT_HEAD_BYTES + (size_t)n * sizeof(u32)));
    if (c->split_words) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipFree(c->split_words);
        if (e != hipSuccess) { (void)hipFree(p); return -(int)e; }
    }
    c->split_words = p; c->split_cap = n;
    return 0;
}

// count -> scan -> fill on one stream, as bvh_intersect_all; every argument is checked before anything is enqueued, so an error writes nothing.  Whether the fill
// runs is decided on the device (split.hip); the host only waits when the caller asks for the total.  The arena is not touched: the call needs no tree
int bvh_split_refs(bvh_ctx* c, const bvh_build_input* in, uint32_t n, float sa_max, uint32_t max_depth, uint32_t* d_offsets, bvh_aabb* d_ref_boxes,
                   uint32_t* d_ref_prims, uint64_t capacity, uint64_t* total_out) {
    if (!c || !in || !d_offsets) return BVH_E_INVALID_ARG;
    if (stage_extents_valid(in)) return BVH_E_INVALID_ARG;
    if (n == 0 || n >= (1u << 30)) return BVH_E_INVALID_ARG;
    if (!(sa_max >= 0.0f)) return BVH_E_INVALID_ARG;          // (NaN or negative)
    if (max_depth > (uint32_t)BVH_SPLIT_MAX_DEPTH) return BVH_E_INVALID_ARG;
    if ((d_ref_boxes == nullptr) != (d_ref_prims == nullptr)) return BVH_E_INVALID_ARG;
    {   // the output ranges may not overlap each other, d_offsets or the input
        Range rs[5] = { Range(d_offsets, ((uint64_t)n + 1u) * sizeof(u32)), fill_range(d_ref_boxes, capacity, sizeof(bvh_aabb)), fill_range(d_ref_prims, capacity, sizeof(u32)) };
        if (!disjoint(rs, 3, 3 + mesh_ranges(*in, n, rs + 3))) return BVH_E_INVALID_ARG;
    }
    Bind b(c->device);
    int r = ensure_split_words(c, n); if (r) return r;
    hipStream_t s = c->stream;
    Install install(c);
    u64* const total = reinterpret_cast<u64*>(c->split_words);
    u32* const heavy_count = reinterpret_cast<u32*>(c->split_words + 8);
    u64* const sums = reinterpret_cast<u64*>(c->split_words + 64);
    u32* const heavy_list = reinterpret_cast<u32*>(c->split_words + SPLIT_HEAD_BYTES);
    hipError_t e = hipMemsetAsync(c->split_words, 0, 16, s);
    if (e == hipSuccess) {
        launch_split_count(s, (int)in->tri_format, in->d_tris, in->d_vertices, in->d_indices, in->n_vertices, n, sa_max, max_depth, d_offsets, heavy_list, heavy_count,
                           sums, total);
        if (d_ref_boxes)
            launch_split_fill(s, (int)in->tri_format, in->d_tris, in->d_vertices, in->d_indices, in->n_vertices, n, sa_max, max_depth, d_offsets, d_ref_boxes,
                              d_ref_prims, capacity, total, heavy_list, heavy_count);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return herr(e);
    install.mark();
    return total_out ? read_total(c, total, total_out) : 0;
}

// ---- batched small-mesh builds (no working counterpart in the reference: src/BatchedBuildKernel.h:218-312 is what this was meant to be) ------------------------------
static_assert(MANY_MAX == BVH_MANY_LDS_MAX_PRIMS, "kernels.hpp MANY_MAX is the header's BVH_MANY_LDS_MAX_PRIMS");
namespace {
struct ManyLayout { uint64_t total = 0; uint32_t n_class[4] = {0, 0, 0, 0}; uint32_t n_large = 0, max_large = 0; };
inline int many_class(uint32_t count) { return count <= 64u ? 0 : count <= 128u ? 1 : count <= 256u ? 2 : count <= (uint32_t)MANY_MAX ? 3 : 4; }
inline bool many_algo_ok(bvh_algo algo) { return algo == BVH_LBVH_SINGLEPASS || algo == BVH_LBVH_TWOPASS; }
// the input's part of the checks bvh_build_many, bvh_build_many_ploc and their *_tree calls share: format, ranges (in and h_meshes are not NULL)
int many_check_input(const bvh_build_input* in, uint32_t n_tris, const bvh_mesh_range* h_meshes, uint32_t n_meshes, ManyLayout* lay) {
    if (n_meshes == 0 || in->morton_bits != 30 || stage_extents_valid(in)) return BVH_E_INVALID_ARG;
    ManyLayout l;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        const uint32_t first = h_meshes[m].first, count = h_meshes[m].count;
        if (count < 2 || (uint64_t)first + count > (uint64_t)n_tris) return BVH_E_INVALID_ARG;
        if (in->tri_format == BVH_TRI_PACKED36 && (first & 3u)) return BVH_E_INVALID_ARG;      // (a consumer reads the slice's records with 16-byte loads)
        l.total += count;
        if (l.total >= (1ull << 30)) return BVH_E_INVALID_ARG;
        const int k = many_class(count);
        if (k < 4) ++l.n_class[k]; else { ++l.n_large; if (count > l.max_large) l.max_large = count; }
    }
    if (lay) *lay = l;
    return 0;
}
int many_check(bvh_algo algo, const bvh_build_input* in, uint32_t n_tris, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_out* out, ManyLayout* lay) {
    if (!in || !h_meshes || !out || n_meshes == 0 || !many_algo_ok(algo)) return BVH_E_INVALID_ARG;
    if (!out->d_nodes || !out->d_prim_aabbs || !out->d_scene_extents || !out->d_roots) return BVH_E_INVALID_ARG;
    return many_check_input(in, n_tris, h_meshes, n_meshes, lay);
}
// six output arrays, then the input's one or two: an output may overlap neither another output nor the input
inline bool many_overlap(Range rs[8], const bvh_build_input* in, uint32_t n_tris) { return !disjoint(rs, 6, 6 + mesh_ranges(*in, n_tris, rs + 6)); }
// the output arrays of either call: LBVH (bvh_many_out: leaves NULL, mesh m's 2n-1 node records from record 2*out_off - m) or PLOC++ (bvh_many_ploc_out: roots NULL,
// n-1 node records from record out_off - m)
struct ManyOutAny { void* nodes; void* leaves; void* boxes; void* scenes; uint32_t* roots; uint32_t* skeys; uint32_t* svals; };
} // namespace

// what bvh_build_many and bvh_build_many_ploc do once their arguments are checked
static int many_build(bvh_ctx* c, bvh_algo algo, const bvh_build_input* in, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const ManyOutAny& o, const ManyLayout& lay,
                      bvh_timings* tm) {
    const bool ploc = algo == BVH_PLOCPP, karras = algo == BVH_LBVH_TWOPASS;
    int r = 0;
    Bind b(c->device);
    hipStream_t s = c->stream;
    const uint32_t n_small = n_meshes - lay.n_large;
    if (n_small > c->many_cap) {                              // (grown outside the arena; the old table may still be read by a launch on the stream)
        uint4* d = nullptr; uint4* h = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), (size_t)n_small * sizeof(uint4)));
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h), (size_t)n_small * sizeof(uint4), hipHostMallocDefault);
        if (e == hipSuccess && !c->many_ev) e = hipEventCreateWithFlags(&c->many_ev, hipEventDisableTiming);
        if (e == hipSuccess && c->many_items) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(d); if (h) (void)hipHostFree(h); return -(int)e; }
        if (c->many_items) { (void)hipFree(c->many_items); (void)hipHostFree(c->many_host); }
        c->many_items = d; c->many_host = h; c->many_cap = n_small;
    } else if (n_small) HIP_TRY(hipEventSynchronize(c->many_ev));   // the previous call's copy has read the pinned words
    if (lay.n_large) { r = ensure_capacity(c, lay.max_large); if (r) return r; }
    Install install(c);
    const bool prof = c->profiling && install.sampled;
    if (prof) HIP_TRY(hipEventRecord(c->ev[5], s));
    if (n_small) {
        uint32_t at[4] = { 0u, lay.n_class[0], lay.n_class[0] + lay.n_class[1], lay.n_class[0] + lay.n_class[1] + lay.n_class[2] };
        uint32_t off = 0;
        for (uint32_t m = 0; m < n_meshes; ++m) {
            const int k = many_class(h_meshes[m].count);
            if (k < 4) c->many_host[at[k]++] = make_uint4(h_meshes[m].first, h_meshes[m].count, off, m);
            off += h_meshes[m].count;
        }
        HIP_TRY(hipMemcpyAsync(c->many_items, c->many_host, (size_t)n_small * sizeof(uint4), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c->many_ev, s));
        if (ploc) {
            ManyPlocArgs a;
            a.tris = in->d_tris; a.verts = in->d_vertices; a.idx = in->d_indices; a.n_verts = in->n_vertices;
            a.boxes = static_cast<bvh_aabb*>(o.boxes); a.scenes = static_cast<bvh_aabb*>(o.scenes); a.nodes = static_cast<bvh2_node*>(o.nodes);
            a.leaves = static_cast<bvh_primref*>(o.leaves); a.skeys = o.skeys; a.svals = o.svals;
            launch_many_ploc(s, a, (int)in->tri_format, c->many_items, lay.n_class);
        } else {
            ManyArgs a;
            a.tris = in->d_tris; a.verts = in->d_vertices; a.idx = in->d_indices; a.n_verts = in->n_vertices;
            a.boxes = static_cast<bvh_aabb*>(o.boxes); a.scenes = static_cast<bvh_aabb*>(o.scenes); a.nodes = static_cast<bvh2_node*>(o.nodes);
            a.roots = o.roots; a.skeys = o.skeys; a.svals = o.svals;
            launch_many(s, a, (int)in->tri_format, karras, c->many_items, lay.n_class);
        }
        HIP_TRY(hipGetLastError());
        install.mark();
    }
    install.end();                                            // (the large meshes' builds tick and record for themselves)
    if (lay.n_large) {                                        // the ordinary build on the ctx (its arena, its read-backs), one mesh after another, copied to the slice
        uint32_t off = 0;
        for (uint32_t m = 0; m < n_meshes; ++m) {
            const uint32_t first = h_meshes[m].first, count = h_meshes[m].count;
            if (many_class(count) == 4) {
                bvh_build_input sub = *in;
                if (in->tri_format == BVH_TRI_INDEXED) sub.d_indices = static_cast<const char*>(in->d_indices) + 12ull * first;
                else sub.d_tris = static_cast<const char*>(in->d_tris) + (in->tri_format == BVH_TRI_PADDED64 ? 64ull : 36ull) * first;
                bvh_result t;
                r = build_impl(c, algo, &sub, count, &t, nullptr); if (r) return r;
                if (ploc) {
                    launch_copy_bytes(s, static_cast<char*>(o.nodes) + ((uint64_t)off - m) * sizeof(bvh2_node), t.d_nodes, (uint64_t)(count - 1u) * sizeof(bvh2_node));
                    launch_copy_bytes(s, static_cast<char*>(o.leaves) + (uint64_t)off * sizeof(bvh_primref), t.d_leaves, (uint64_t)count * sizeof(bvh_primref));
                } else launch_copy_bytes(s, static_cast<char*>(o.nodes) + (2ull * off - m) * sizeof(bvh2_node), t.d_nodes, (2ull * count - 1u) * sizeof(bvh2_node));
                launch_copy_bytes(s, static_cast<char*>(o.boxes) + (uint64_t)off * sizeof(bvh_aabb), t.d_prim_aabbs, (uint64_t)count * sizeof(bvh_aabb));
                launch_copy_bytes(s, static_cast<char*>(o.scenes) + (uint64_t)m * sizeof(bvh_aabb), t.d_scene_extent, sizeof(bvh_aabb));
                if (o.skeys) launch_copy_bytes(s, o.skeys + off, t.d_sorted_keys, (uint64_t)count * sizeof(u32));
                if (o.svals) launch_copy_bytes(s, o.svals + off, t.d_sorted_vals, (uint64_t)count * sizeof(u32));
                if (karras) HIP_TRY(hipMemsetAsync(o.roots + m, 0, sizeof(u32), s));
                else if (!ploc) launch_copy_bytes(s, o.roots + m, c->small, sizeof(u32));
                HIP_TRY(hipGetLastError());
            }
            off += count;
        }
    }
    if (prof) HIP_TRY(hipEventRecord(c->ev[6], s));
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->bytes_algorithmic = algorithmic_bytes(algo, (uint32_t)lay.total);
        tm->sampled = prof ? 1u : 0u;
        if (prof) {
            HIP_TRY(hipEventSynchronize(c->ev[6]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_build, c->ev[5], c->ev[6]));
            tm->ms_total = tm->ms_build;
        }
    }
    return 0;
}

int bvh_build_many(bvh_ctx* c, bvh_algo algo, const bvh_build_input* in, uint32_t n_tris, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_out* out,
                   bvh_timings* tm) {
    if (!c) return BVH_E_INVALID_ARG;
    ManyLayout lay;
    int r = many_check(algo, in, n_tris, h_meshes, n_meshes, out, &lay); if (r) return r;
    Range rs[8] = {
        Range(out->d_nodes, (2ull * lay.total - n_meshes) * sizeof(bvh2_node)), Range(out->d_prim_aabbs, lay.total * sizeof(bvh_aabb)),
        Range(out->d_scene_extents, (uint64_t)n_meshes * sizeof(bvh_aabb)), Range(out->d_roots, (uint64_t)n_meshes * sizeof(u32)),
        Range(out->d_sorted_keys, lay.total * sizeof(u32)), Range(out->d_sorted_vals, lay.total * sizeof(u32)) };
    if (many_overlap(rs, in, n_tris)) return BVH_E_INVALID_ARG;
    const ManyOutAny o = { out->d_nodes, nullptr, out->d_prim_aabbs, out->d_scene_extents, out->d_roots, out->d_sorted_keys, out->d_sorted_vals };
    return many_build(c, algo, in, h_meshes, n_meshes, o, lay, tm);
}

int bvh_build_many_ploc(bvh_ctx* c, bvh_algo algo, const bvh_build_input* in, uint32_t n_tris, const bvh_mesh_range* h_meshes, uint32_t n_meshes,
                        const bvh_many_ploc_out* out, bvh_timings* tm) {
    if (!c || !in || !h_meshes || !out || algo != BVH_PLOCPP) return BVH_E_INVALID_ARG;
    if (!out->d_nodes || !out->d_leaves || !out->d_prim_aabbs || !out->d_scene_extents) return BVH_E_INVALID_ARG;
    ManyLayout lay;
    int r = many_check_input(in, n_tris, h_meshes, n_meshes, &lay); if (r) return r;
    Range rs[8] = {
        Range(out->d_nodes, (lay.total - n_meshes) * sizeof(bvh2_node)), Range(out->d_leaves, lay.total * sizeof(bvh_primref)),
        Range(out->d_prim_aabbs, lay.total * sizeof(bvh_aabb)), Range(out->d_scene_extents, (uint64_t)n_meshes * sizeof(bvh_aabb)),
        Range(out->d_sorted_keys, lay.total * sizeof(u32)), Range(out->d_sorted_vals, lay.total * sizeof(u32)) };
    if (many_overlap(rs, in, n_tris)) return BVH_E_INVALID_ARG;
    const ManyOutAny o = { out->d_nodes, out->d_leaves, out->d_prim_aabbs, out->d_scene_extents, nullptr, out->d_sorted_keys, out->d_sorted_vals };
    return many_build(c, algo, in, h_meshes, n_meshes, o, lay, tm);
}

int bvh_many_tree(bvh_algo algo, const bvh_build_input* in, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_out* out, uint32_t m,
                  const uint32_t* h_roots, bvh_result* tree_out, bvh_build_input* tris_out) {
    if (!in || !h_meshes || !out || !tree_out || !tris_out || m >= n_meshes || !many_algo_ok(algo)) return BVH_E_INVALID_ARG;
    if (algo == BVH_LBVH_SINGLEPASS && !h_roots) return BVH_E_INVALID_ARG;
    if (in->morton_bits != 30 || stage_extents_valid(in)) return BVH_E_INVALID_ARG;
    if (!out->d_nodes || !out->d_prim_aabbs || !out->d_scene_extents) return BVH_E_INVALID_ARG;
    uint64_t off = 0;
    for (uint32_t k = 0; k < m; ++k) off += h_meshes[k].count;
    const uint32_t first = h_meshes[m].first, count = h_meshes[m].count;
    if (count < 2 || off + count >= (1ull << 30)) return BVH_E_INVALID_ARG;
    if (in->tri_format == BVH_TRI_PACKED36 && (first & 3u)) return BVH_E_INVALID_ARG;
    bvh_result t; std::memset(&t, 0, sizeof t);
    t.d_nodes = static_cast<char*>(out->d_nodes) + (2ull * off - m) * sizeof(bvh2_node);
    t.d_prim_aabbs = static_cast<char*>(out->d_prim_aabbs) + off * sizeof(bvh_aabb);
    t.d_scene_extent = static_cast<char*>(out->d_scene_extents) + (uint64_t)m * sizeof(bvh_aabb);
    t.d_sorted_keys = out->d_sorted_keys ? out->d_sorted_keys + off : nullptr;
    t.d_sorted_vals = out->d_sorted_vals ? out->d_sorted_vals + off : nullptr;
    t.root = algo == BVH_LBVH_TWOPASS ? 0u : h_roots[m];
    t.n_internal = count - 1; t.n_leaves = count; t.layout = 0; t.key_bits = 32;
    bvh_build_input ti = *in;
    switch (in->tri_format) {
        case BVH_TRI_PADDED64: ti.d_tris = static_cast<const char*>(in->d_tris) + 64ull * first; t.d_tris = ti.d_tris; break;
        case BVH_TRI_PACKED36: ti.d_tris = static_cast<const char*>(in->d_tris) + 36ull * first; break;
        default:               ti.d_indices = static_cast<const char*>(in->d_indices) + 12ull * first; break;
    }
    *tree_out = t; *tris_out = ti;
    return 0;
}

int bvh_many_ploc_tree(bvh_algo algo, const bvh_build_input* in, const bvh_mesh_range* h_meshes, uint32_t n_meshes, const bvh_many_ploc_out* out, uint32_t m,
                       bvh_result* tree_out, bvh_build_input* tris_out) {
    if (!in || !h_meshes || !out || !tree_out || !tris_out || m >= n_meshes || algo != BVH_PLOCPP) return BVH_E_INVALID_ARG;
    if (in->morton_bits != 30 || stage_extents_valid(in)) return BVH_E_INVALID_ARG;
    if (!out->d_nodes || !out->d_leaves || !out->d_prim_aabbs || !out->d_scene_extents) return BVH_E_INVALID_ARG;
    uint64_t off = 0;
    for (uint32_t k = 0; k < m; ++k) off += h_meshes[k].count;
    const uint32_t first = h_meshes[m].first, count = h_meshes[m].count;
    if (count < 2 || off + count >= (1ull << 30)) return BVH_E_INVALID_ARG;
    if (in->tri_format == BVH_TRI_PACKED36 && (first & 3u)) return BVH_E_INVALID_ARG;
    bvh_result t; std::memset(&t, 0, sizeof t);
    t.d_nodes = static_cast<char*>(out->d_nodes) + (off - m) * sizeof(bvh2_node);
    t.d_leaves = static_cast<char*>(out->d_leaves) + off * sizeof(bvh_primref);
    t.d_prim_aabbs = static_cast<char*>(out->d_prim_aabbs) + off * sizeof(bvh_aabb);
    t.d_scene_extent = static_cast<char*>(out->d_scene_extents) + (uint64_t)m * sizeof(bvh_aabb);
    t.d_sorted_keys = out->d_sorted_keys ? out->d_sorted_keys + off : nullptr;
    t.d_sorted_vals = out->d_sorted_vals ? out->d_sorted_vals + off : nullptr;
    t.root = 0u; t.n_internal = count - 1; t.n_leaves = count; t.layout = 1; t.key_bits = 32;
    bvh_build_input ti = *in;
    switch (in->tri_format) {
        case BVH_TRI_PADDED64: ti.d_tris = static_cast<const char*>(in->d_tris) + 64ull * first; t.d_tris = ti.d_tris; break;
        case BVH_TRI_PACKED36: ti.d_tris = static_cast<const char*>(in->d_tris) + 36ull * first; break;
        default:               ti.d_indices = static_cast<const char*>(in->d_indices) + 12ull * first; break;
    }
    *tree_out = t; *tris_out = ti;
    return 0;
}

// every leaf's primitive index through a map.  Topology and boxes stay: the ctx's cached parent plan remains valid (tree_serial is not bumped); the cached leaf
// map of bvh_refit_subset describes the old indices and is dropped
int bvh_remap_leaves(bvh_ctx* c, bvh_result* io, const uint32_t* d_map, uint32_t n_map) {
    int r = refit_check(c, io); if (r) return r;
    if (!d_map) return BVH_E_INVALID_ARG;
    const uint32_t n = io->n_leaves;
    {   // the map may not overlap the leaf records
        const char* w = io->layout == 0 ? (const char*)io->d_nodes + (uint64_t)(n - 1) * sizeof(bvh2_node) : (const char*)io->d_leaves;
        const uint64_t w_bytes = (uint64_t)n * (io->layout == 0 ? sizeof(bvh2_node) : sizeof(bvh_primref));
        if (crosses(Range(d_map, (uint64_t)n_map * sizeof(u32)), Range(w, w_bytes))) return BVH_E_INVALID_ARG;
    }
    Bind b(c->device);
    Install install(c);
    c->map_serial = 0;
    launch_remap_leaves(c->stream, io->d_nodes, io->d_leaves, (int)io->layout, n, d_map, n_map);
    HIP_TRY(hipGetLastError());
    install.mark();
    return 0;
}

// ---- tree optimisation (no counterpart in the reference) ----------------------------------------------------------------------------------------
// every argument is checked before anything is enqueued: an error writes nothing.  The arena is never re-allocated (io may point into it).  The rounds keep
// parent[] right for the new topology, so the cached plan of the ctx's own tree stays valid (tree_serial is not bumped); caller-owned arrays leave a plan of
// THEIR tree in `parent`, which the ctx's own tree does not use (plan_serial 0, as after a refit of caller-owned arrays).
int bvh_optimize(bvh_ctx* c, bvh_result* io, uint32_t rounds, bvh_timings* tm) {
    if (!c || !io) return BVH_E_INVALID_ARG;
    if (!tree_valid(io)) return BVH_E_INVALID_ARG;
    const uint32_t n = io->n_leaves;
    if (rounds < 1u || rounds > 8u) return BVH_E_INVALID_ARG;
    if (n > c->cap) return BVH_E_INVALID_ARG;                 // (parent / flags scratch is sized by the capacity: bvh_ctx_reserve first)
    Bind b(c->device);
    hipStream_t s = c->stream;
    Install install(c);
    const bool prof = c->profiling && install.sampled;
    if (prof) HIP_TRY(hipEventRecord(c->ev[1], s));
    int r = begin_emit(c); if (r) return r;
    const bool own = io->d_nodes == c->nodes;
    if (!own || c->plan_serial != c->tree_serial || c->plan_n != n || c->plan_root != io->root) {
        launch_refit_plan(s, io->d_nodes, n, io->root, c->parent);
        c->plan_serial = own ? c->tree_serial : 0; c->plan_n = n; c->plan_root = io->root;
    }
    uint32_t ran = 0;
    for (uint32_t k = 0; k < rounds && (7u << k) <= n; ++k, ++ran)       // (a round whose gamma exceeds n has no treelet root: not launched)
        launch_optimize(s, io->d_nodes, io->d_leaves, (int)io->layout, n, 7u << k, c->parent, c->flags);
    r = end_emit(c); if (r) { c->plan_serial = 0; return r; }
    install.mark();
    if (prof) HIP_TRY(hipEventRecord(c->ev[4], s));
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->bytes_algorithmic = 80ull * n * ran;     // nominal
        tm->sampled = prof ? 1u : 0u;
        if (prof) {
            HIP_TRY(hipEventSynchronize(c->ev[4]));
            HIP_TRY(hipEventElapsedTime(&tm->ms_build, c->ev[1], c->ev[4]));
            tm->ms_total = tm->ms_build;
        }
    }
    return 0;
}

// ---- instanced scenes (no counterpart in the reference) -----------------------------------------------------------------------------------------
int bvh_scene_create(bvh_ctx* c, bvh_scene** out) {
    if (!c || !out) return BVH_E_INVALID_ARG;
    bvh_scene* sc = new (std::nothrow) bvh_scene();
    if (!sc) return BVH_E_INTERNAL;
    sc->ctx = c;
    *out = sc;
    return 0;
}

void bvh_scene_destroy(bvh_scene* sc) {
    if (!sc) return;
    if (sc->mem) { Bind b(sc->ctx->device); hipStreamSynchronize(sc->ctx->stream); hipFree(sc->mem); if (sc->wmem) hipFree(sc->wmem); }
    delete sc;
}

namespace {
// one bvh_blas -> its device descriptor; BVH_E_INVALID_ARG for what bvh_intersect would reject and for arrays inside the ctx's arena / triangle staging buffer
int blas_descriptor(const bvh_ctx* c, const bvh_blas& in, SceneBlas& d) {
    const bvh_result& t = in.tree;
    const uint32_t n = t.n_leaves;
    if (!tree_valid(&t) || n >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input tri = in.tris;
    if (tri.tri_format == BVH_TRI_PADDED64 && !tri.d_tris) tri.d_tris = t.d_tris;
    if (stage_extents_valid(&tri)) return BVH_E_INVALID_ARG;
    const Range own[2] = { Range(c->arena, c->arena_bytes), Range(c->tris, (uint64_t)c->tris_cap * sizeof(bvh_triangle)) };
    Range arrays[4];
    int k = tree_ranges(&t, arrays);
    k += mesh_ranges(tri, n, arrays + k);
    for (int a = 0; a < k; ++a) if (crosses(arrays[a], own, 2)) return BVH_E_INVALID_ARG;
    std::memset(&d, 0, sizeof d);
    d.nodes = t.d_nodes; d.leaves = t.layout == 1 ? t.d_leaves : nullptr; d.tris = tri.tri_format == BVH_TRI_INDEXED ? tri.d_vertices : tri.d_tris;
    d.idx = tri.tri_format == BVH_TRI_INDEXED ? tri.d_indices : nullptr;
    d.n = n; d.root = t.root; d.layout = t.layout; d.fmt = tri.tri_format; d.nv = tri.n_vertices;
    return 0;
}
// instance records -> the scene's copy (host or device source), then k_instance_boxes
int scene_instances(bvh_scene* sc, const bvh_instance* instances, int on_device) {
    hipStream_t s = sc->ctx->stream;
    HIP_TRY(hipMemcpyAsync(sc->inst_in, instances, (size_t)sc->n_inst * sizeof(bvh_instance), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (!on_device) HIP_TRY(hipStreamSynchronize(s));        // (host records: read before the call returns)
    launch_instance_boxes(s, sc->inst_in, sc->n_inst, sc->blas, sc->n_blas, sc->inst, sc->wbox);
    return herr(hipGetLastError());
}
} // namespace

int bvh_scene_build(bvh_scene* sc, bvh_algo algo, const bvh_blas* blas, uint32_t n_blas, const bvh_instance* instances, uint32_t n_inst, int on_device,
                    bvh_timings* tm) {
    if (!sc || !blas || !instances || n_blas == 0 || n_inst == 0 || (int)algo < 0 || (int)algo > 3) return BVH_E_INVALID_ARG;
    if (n_inst >= (1u << 30)) return BVH_E_TOO_LARGE;
    bvh_ctx* c = sc->ctx;
    std::vector<SceneBlas> desc(n_blas);
    uint64_t plan_words = 0;
    for (uint32_t k = 0; k < n_blas; ++k) {
        const int r = blas_descriptor(c, blas[k], desc[k]); if (r) return r;
        plan_words += 2ull * desc[k].n - 1;
    }
    Bind b(c->device);
    if (tm) std::memset(tm, 0, sizeof *tm);
    // carve the scene's memory (freed and re-made on every build: the BLAS set and the instance count may change)
    const size_t n = n_inst;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_blas = take(n_blas * sizeof(SceneBlas)), o_in = take(n * sizeof(bvh_instance)), o_inst = take(n * sizeof(SceneInst)), o_wbox = take(n * sizeof(bvh_aabb));
    const size_t o_tnodes = take((2 * n - 1) * sizeof(bvh2_node)), o_tleaves = take(n * sizeof(bvh_primref)), o_tparent = take((2 * n - 1) * sizeof(u32));
    const size_t o_flags = take(n * sizeof(u32)), o_over = take(sizeof(u32)), o_plans = take(plan_words * sizeof(u32));
    sc->built = false;
    sc->wind_blas_ok = sc->wind_ok = false;                      // (the winding moments describe the old BLAS set: discarded with it)
    if (sc->mem) {
        HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(sc->mem)); sc->mem = nullptr;
        if (sc->wmem) { HIP_TRY(hipFree(sc->wmem)); sc->wmem = nullptr; }
    }
    sc->blas_n.resize(n_blas);
    for (uint32_t k = 0; k < n_blas; ++k) sc->blas_n[k] = desc[k].n;
    HIP_TRY(hipMalloc(&sc->mem, off));
    char* m = sc->mem;
    sc->blas = reinterpret_cast<SceneBlas*>(m + o_blas); sc->inst_in = reinterpret_cast<bvh_instance*>(m + o_in); sc->inst = reinterpret_cast<SceneInst*>(m + o_inst);
    sc->wbox = reinterpret_cast<bvh_aabb*>(m + o_wbox); sc->tnodes = reinterpret_cast<bvh2_node*>(m + o_tnodes); sc->tleaves = reinterpret_cast<bvh_primref*>(m + o_tleaves);
    sc->tparent = reinterpret_cast<u32*>(m + o_tparent); sc->flags = reinterpret_cast<u32*>(m + o_flags); sc->overflow = reinterpret_cast<u32*>(m + o_over);
    sc->n_blas = n_blas; sc->n_inst = n_inst;
    hipStream_t s = c->stream;
    // the descriptors (each with its slot of the plans), copied before anything is enqueued: a blocking copy, so that an early return cannot leave a copy
    // from `desc` queued; then every BLAS's parent plan (the stackless pass)
    u32* const plans = reinterpret_cast<u32*>(m + o_plans);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_blas; ++k) { desc[k].parent = plans + at; at += 2ull * desc[k].n - 1; }
    HIP_TRY(hipMemcpy(sc->blas, desc.data(), n_blas * sizeof(SceneBlas), hipMemcpyHostToDevice));
    for (uint32_t k = 0; k < n_blas; ++k) launch_refit_plan(s, desc[k].nodes, desc[k].n, desc[k].root, const_cast<u32*>(desc[k].parent));
    HIP_TRY(hipMemsetAsync(sc->flags, 0xFF, n * sizeof(u32), s));
    int r = scene_instances(sc, instances, on_device); if (r) return r;
    sc->troot = 0; sc->tlayout = (algo == BVH_PLOCPP || algo == BVH_HPLOC) ? 1u : 0u;
    if (n_inst >= 2) {
        // the top-level tree: built in the ctx's arena over the world boxes, copied out, and its own plan
        bvh_result t;
        r = bvh_build_boxes(c, algo, sc->wbox, n_inst, 30, &t, tm); if (r) return r;
        sc->troot = t.root; sc->tlayout = t.layout;
        HIP_TRY(hipMemcpyAsync(sc->tnodes, t.d_nodes, (t.layout == 0 ? 2 * n - 1 : n - 1) * sizeof(bvh2_node), hipMemcpyDeviceToDevice, s));
        if (t.layout == 1) HIP_TRY(hipMemcpyAsync(sc->tleaves, t.d_leaves, n * sizeof(bvh_primref), hipMemcpyDeviceToDevice, s));
        launch_refit_plan(s, sc->tnodes, n_inst, sc->troot, sc->tparent);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                          // (bvh_scene_build is blocking: errors of the enqueued work surface here)
    sc->built = true;
    return 0;
}

int bvh_scene_update(bvh_scene* sc, const bvh_instance* instances, int on_device, bvh_timings* tm) {
    if (!sc || !instances || !sc->built) return BVH_E_INVALID_ARG;
    bvh_ctx* c = sc->ctx;
    Bind b(c->device);
    hipStream_t s = c->stream;
    const bool prof = c->profiling;
    if (prof) HIP_TRY(hipEventRecord(c->ev[0], s));
    sc->wind_ok = false;                                         // (the maps, instance moments and top-level moments are stale; the BLAS moments are not)
    int r = scene_instances(sc, instances, on_device); if (r) return r;
    if (sc->n_inst >= 2) launch_refit_climb(s, sc->wbox, sc->tnodes, sc->tleaves, (int)sc->tlayout, sc->n_inst, sc->tparent, sc->flags);
    HIP_TRY(hipGetLastError());
    if (prof) HIP_TRY(hipEventRecord(c->ev[4], s));
    if (tm) {
        std::memset(tm, 0, sizeof *tm);
        tm->sampled = prof ? 1u : 0u;
        if (prof) { HIP_TRY(hipEventSynchronize(c->ev[4])); HIP_TRY(hipEventElapsedTime(&tm->ms_build, c->ev[0], c->ev[4])); tm->ms_total = tm->ms_build; }
    }
    return 0;
}

int bvh_scene_intersect(bvh_scene* sc, const bvh_ray* d_rays, uint32_t n_rays, bvh_instance_hit* d_hits, int query) {
    if (!sc || !d_rays || !d_hits || !sc->built) return BVH_E_INVALID_ARG;
    if (query != BVH_QUERY_CLOSEST && query != BVH_QUERY_ANY) return BVH_E_INVALID_ARG;
    if (crosses(Range(d_rays, (uint64_t)n_rays * sizeof(bvh_ray)), Range(d_hits, (uint64_t)n_rays * sizeof(bvh_instance_hit)))) return BVH_E_INVALID_ARG;
    if (n_rays == 0) return 0;
    return query_tail(sc->ctx, nullptr, sc->overflow, [&](hipStream_t s, u32* overflow) { launch_scene_intersect(s, query, scene_query(sc, d_rays, n_rays, d_hits, overflow)); });
}

int bvh_scene_closest_point(bvh_scene* sc, const bvh_point_query* d_points, uint32_t n_points, bvh_instance_point_hit* d_hits, int query) {
    if (!sc || !d_points || !d_hits || !sc->built) return BVH_E_INVALID_ARG;
    if (query != BVH_QUERY_CLOSEST && query != BVH_QUERY_ANY) return BVH_E_INVALID_ARG;
    if (crosses(Range(d_points, (uint64_t)n_points * sizeof(bvh_point_query)), Range(d_hits, (uint64_t)n_points * sizeof(bvh_instance_point_hit)))) return BVH_E_INVALID_ARG;
    if (n_points == 0) return 0;
    return query_tail(sc->ctx, nullptr, sc->overflow, [&](hipStream_t s, u32* overflow) { launch_scene_closest_point(s, query, scene_query(sc, d_points, n_points, d_hits, overflow)); });
}

// bvh_scene_closest_point's scene and bvh_knn's argument rules; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_knn(bvh_scene* sc, const bvh_point_query* d_points, uint32_t n_points, uint32_t k, bvh_instance_knn_hit* d_hits, uint32_t* d_counts) {
    if (!sc || !d_points || !d_hits || !sc->built) return BVH_E_INVALID_ARG;
    if (k == 0u || k > (uint32_t)BVH_KNN_MAX_K) return BVH_E_INVALID_ARG;
    if ((uint64_t)n_points * k >= (1ull << 32)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_points, (uint64_t)n_points * sizeof(bvh_point_query)), Range(d_hits, (uint64_t)n_points * k * sizeof(bvh_instance_knn_hit)),
                          Range(d_counts, (uint64_t)n_points * sizeof(u32)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    if (n_points == 0) return 0;
    return query_tail(sc->ctx, nullptr, sc->overflow, [&](hipStream_t s, u32* overflow) {
        SceneQuery q = scene_query(sc, d_points, n_points, d_hits, overflow);
        q.counts = d_counts; q.k = k;
        launch_scene_knn(s, q);
    });
}

// bvh_scene_intersect's scene and bvh_intersect_all's tail (the ctx's words: a scene is bound to one ctx and one stream, whose calls are ordered); every argument
// is checked before anything is enqueued, so an error writes nothing
int bvh_scene_intersect_all(bvh_scene* sc, const bvh_ray* d_rays, uint32_t n_rays, uint32_t flags, uint32_t* d_offsets, bvh_instance_hit* d_hits,
                            uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_rays || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_HITS_SORTED) return BVH_E_INVALID_ARG;
    if (n_rays >= (1u << 30)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_rays, (uint64_t)n_rays * sizeof(bvh_ray)), Range(d_offsets, ((uint64_t)n_rays + 1u) * sizeof(u32)), fill_range(d_hits, capacity, sizeof(bvh_instance_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(sc->ctx, nullptr, n_rays, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, d_rays, n_rays, d_hits, overflow);
        const SceneHits h{ d_offsets, d_hits, total, capacity };
        launch_scene_hits_count(s, q, h, sc->ctx->overlap_sums, total);
        if (d_hits) { q.overflow = overflow + 1; launch_scene_hits_fill(s, (flags & BVH_HITS_SORTED) ? 1 : 0, q, h); }
    });
}

// bvh_scene_closest_point's scene and points, bvh_scene_intersect_all's tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_radius_search(bvh_scene* sc, const bvh_point_query* d_points, uint32_t n_points, uint32_t flags, uint32_t* d_offsets, bvh_instance_knn_hit* d_hits,
                            uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_points || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_RADIUS_SORTED) return BVH_E_INVALID_ARG;
    if (n_points >= (1u << 30)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_points, (uint64_t)n_points * sizeof(bvh_point_query)), Range(d_offsets, ((uint64_t)n_points + 1u) * sizeof(u32)), fill_range(d_hits, capacity, sizeof(bvh_instance_knn_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(sc->ctx, nullptr, n_points, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, d_points, n_points, d_hits, overflow);
        const SceneHits h{ d_offsets, d_hits, total, capacity };
        launch_scene_radius_count(s, q, h, sc->ctx->overlap_sums, total);
        if (d_hits) { q.overflow = overflow + 1; launch_scene_radius_fill(s, (flags & BVH_RADIUS_SORTED) ? 1 : 0, q, h); }
    });
}

// bvh_overlap's query boxes on a scene, bvh_scene_radius_search's tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_overlap(bvh_scene* sc, const bvh_aabb* d_boxes, uint32_t n_boxes, uint32_t flags, uint32_t* d_offsets, bvh_instance_prim* d_prims,
                      uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_boxes || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_SCENE_OVERLAP_SORTED) return BVH_E_INVALID_ARG;
    if (n_boxes >= (1u << 30)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_boxes, (uint64_t)n_boxes * sizeof(bvh_aabb)), Range(d_offsets, ((uint64_t)n_boxes + 1u) * sizeof(u32)), fill_range(d_prims, capacity, sizeof(bvh_instance_prim)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    return count_fill_tail(sc->ctx, nullptr, n_boxes, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, d_boxes, n_boxes, d_prims, overflow);
        const SceneHits h{ d_offsets, d_prims, total, capacity };
        launch_scene_overlap_count(s, q, h, sc->ctx->overlap_sums, total);
        if (d_prims) { q.overflow = overflow + 1; launch_scene_overlap_fill(s, (flags & BVH_SCENE_OVERLAP_SORTED) ? 1 : 0, q, h); }
    });
}

// bvh_cull's volumes on a scene, bvh_scene_overlap's tail; every argument is checked before anything is enqueued, so an error writes nothing.  The walk is chosen
// here: BVH_CULL_AUTO takes the group walk for few volumes on a scene large enough to fill a workgroup's rounds (kernels.hpp's two constants)
int bvh_scene_cull(bvh_scene* sc, const float* d_planes, uint32_t n_volumes, uint32_t planes_per_volume, int path, uint32_t* d_offsets,
                   bvh_scene_cull_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_planes || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (planes_per_volume < 1u || planes_per_volume > (uint32_t)BVH_CULL_MAX_PLANES) return BVH_E_INVALID_ARG;
    if (path != BVH_CULL_AUTO && path != BVH_CULL_LANE && path != BVH_CULL_GROUP) return BVH_E_INVALID_ARG;
    if (n_volumes >= (1u << 30)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_planes, (uint64_t)n_volumes * planes_per_volume * 4u * sizeof(float)), Range(d_offsets, ((uint64_t)n_volumes + 1u) * sizeof(u32)),
                          fill_range(d_hits, capacity, sizeof(bvh_scene_cull_hit)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    uint32_t largest = 0;
    for (uint32_t n : sc->blas_n) largest = n > largest ? n : largest;
    const bool group = path == BVH_CULL_GROUP || (path == BVH_CULL_AUTO && n_volumes <= SCENE_CULL_AUTO_MAX_VOLUMES &&
                                                  (uint64_t)sc->n_inst + largest >= SCENE_CULL_AUTO_MIN_LEAVES);
    const uint64_t max_pops = (uint64_t)sc->n_inst * ((uint64_t)largest + 2u);      // (every instance's internal nodes and the top level's: a tree expands fewer)
    return count_fill_tail(sc->ctx, nullptr, n_volumes, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, d_planes, n_volumes, d_hits, overflow);
        const SceneHits h{ d_offsets, d_hits, total, capacity };
        launch_scene_cull_count(s, group, q, h, planes_per_volume, max_pops, sc->ctx->overlap_sums, total);
        if (d_hits) { q.overflow = overflow + 1; launch_scene_cull_fill(s, group, q, h, planes_per_volume, max_pops); }
    });
}

// bvh_intersect_tris's query mesh on a scene (or one instance's own triangles, named by index and resolved on the device), bvh_scene_overlap's tail; every
// argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_intersect_tris(bvh_scene* sc, const bvh_build_input* queries, uint32_t n_queries, int mode, uint32_t query_instance, uint32_t flags,
                             uint32_t* d_offsets, bvh_instance_prim* d_prims, uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_SCENE_TRIS_SORTED) return BVH_E_INVALID_ARG;
    if (mode != BVH_SCENE_TRIS_QUERY && mode != BVH_SCENE_TRIS_INSTANCE) return BVH_E_INVALID_ARG;
    if ((mode == BVH_SCENE_TRIS_INSTANCE) != (queries == nullptr)) return BVH_E_INVALID_ARG;     // the world-space mesh, or none in instance mode
    if (mode == BVH_SCENE_TRIS_INSTANCE ? query_instance >= sc->n_inst : query_instance != 0u) return BVH_E_INVALID_ARG;
    if (n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input qin;
    std::memset(&qin, 0, sizeof qin);
    if (queries) { if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG; qin = *queries; }
    {   // the output arrays against each other and against the query mesh
        Range rs[4] = { Range(d_offsets, ((uint64_t)n_queries + 1u) * sizeof(u32)), fill_range(d_prims, capacity, sizeof(bvh_instance_prim)) };
        int k = 2;
        if (queries) k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 2, k)) return BVH_E_INVALID_ARG;
    }
    const SceneTris st{ TrisMesh{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices }, mode, query_instance };
    return count_fill_tail(sc->ctx, nullptr, n_queries, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, nullptr, n_queries, d_prims, overflow);
        const SceneHits h{ d_offsets, d_prims, total, capacity };
        launch_scene_tris_count(s, q, h, st, sc->ctx->overlap_sums, total);
        if (d_prims) { q.overflow = overflow + 1; launch_scene_tris_fill(s, (flags & BVH_SCENE_TRIS_SORTED) ? 1 : 0, q, h, st); }
    });
}

// bvh_closest_tris's query on a scene: bvh_scene_intersect_tris's validation of the query side (in its order), bvh_closest_tris's overlap check of the answers
// against the query mesh, bvh_scene_closest_point's tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_closest_tris(bvh_scene* sc, const bvh_build_input* queries, uint32_t n_queries, int mode, uint32_t query_instance, float radius,
                           bvh_instance_tri_hit* d_hits, int query) {
    if (!sc || !d_hits || !sc->built) return BVH_E_INVALID_ARG;
    if (query != BVH_QUERY_CLOSEST && query != BVH_QUERY_ANY) return BVH_E_INVALID_ARG;
    if (mode != BVH_SCENE_TRIS_QUERY && mode != BVH_SCENE_TRIS_INSTANCE) return BVH_E_INVALID_ARG;
    if ((mode == BVH_SCENE_TRIS_INSTANCE) != (queries == nullptr)) return BVH_E_INVALID_ARG;     // the world-space mesh, or none in instance mode
    if (mode == BVH_SCENE_TRIS_INSTANCE ? query_instance >= sc->n_inst : query_instance != 0u) return BVH_E_INVALID_ARG;
    if (n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input qin;
    std::memset(&qin, 0, sizeof qin);
    if (queries) { if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG; qin = *queries; }
    {   // the answers against the query mesh
        Range rs[3] = { Range(d_hits, (uint64_t)n_queries * sizeof(bvh_instance_tri_hit)) };
        int k = 1;
        if (queries) k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 1, k)) return BVH_E_INVALID_ARG;
    }
    if (n_queries == 0) return 0;
    const SceneTris st{ TrisMesh{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices }, mode, query_instance };
    return query_tail(sc->ctx, nullptr, sc->overflow, [&](hipStream_t s, u32* overflow) {
        launch_scene_closest_tris(s, query, radius, scene_query(sc, nullptr, n_queries, d_hits, overflow), st);
    });
}

// bvh_radius_tris's query on a scene: bvh_scene_intersect_tris's validation block (in its order) with bvh_instance_tri_hit records, bvh_scene_radius_search's
// tail; every argument is checked before anything is enqueued, so an error writes nothing
int bvh_scene_radius_tris(bvh_scene* sc, const bvh_build_input* queries, uint32_t n_queries, int mode, uint32_t query_instance, float radius, uint32_t flags,
                          uint32_t* d_offsets, bvh_instance_tri_hit* d_hits, uint64_t capacity, uint64_t* total_out) {
    if (!sc || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~BVH_SCENE_RADIUS_TRIS_SORTED) return BVH_E_INVALID_ARG;
    if (mode != BVH_SCENE_TRIS_QUERY && mode != BVH_SCENE_TRIS_INSTANCE) return BVH_E_INVALID_ARG;
    if ((mode == BVH_SCENE_TRIS_INSTANCE) != (queries == nullptr)) return BVH_E_INVALID_ARG;     // the world-space mesh, or none in instance mode
    if (mode == BVH_SCENE_TRIS_INSTANCE ? query_instance >= sc->n_inst : query_instance != 0u) return BVH_E_INVALID_ARG;
    if (n_queries >= (1u << 30)) return BVH_E_INVALID_ARG;
    bvh_build_input qin;
    std::memset(&qin, 0, sizeof qin);
    if (queries) { if (stage_extents_valid(queries)) return BVH_E_INVALID_ARG; qin = *queries; }
    {   // the output arrays against each other and against the query mesh
        Range rs[4] = { Range(d_offsets, ((uint64_t)n_queries + 1u) * sizeof(u32)), fill_range(d_hits, capacity, sizeof(bvh_instance_tri_hit)) };
        int k = 2;
        if (queries) k += mesh_ranges(qin, n_queries, rs + k);
        if (!disjoint(rs, 2, k)) return BVH_E_INVALID_ARG;
    }
    const SceneTris st{ TrisMesh{ (int)qin.tri_format, qin.d_tris, qin.d_vertices, qin.d_indices, qin.n_vertices }, mode, query_instance };
    return count_fill_tail(sc->ctx, nullptr, n_queries, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
        SceneQuery q = scene_query(sc, nullptr, n_queries, d_hits, overflow);
        const SceneHits h{ d_offsets, d_hits, total, capacity };
        launch_scene_radius_tris_count(s, radius, q, h, st, sc->ctx->overlap_sums, total);
        if (d_hits) { q.overflow = overflow + 1; launch_scene_radius_tris_fill(s, (flags & BVH_SCENE_RADIUS_TRIS_SORTED) ? 1 : 0, radius, q, h, st); }
    });
}

// bvh_scene_intersect_tris's INSTANCE mode for every instance at once: the row table is made on the device (launch_scene_collide_rows) in front of
// bvh_scene_overlap's tail over row_capacity rows; every argument is checked before anything is enqueued, so an error writes nothing.  rows_out and total_out are
// the only waits
int bvh_scene_collide(bvh_scene* sc, uint32_t flags, uint32_t* d_row_first, uint32_t row_capacity, uint32_t* d_offsets, bvh_instance_prim* d_prims,
                      uint64_t capacity, uint64_t* rows_out, uint64_t* total_out) {
    if (!sc || !d_row_first || !d_offsets || !sc->built) return BVH_E_INVALID_ARG;
    if (flags & ~(BVH_SCENE_COLLIDE_SORTED | BVH_SCENE_COLLIDE_BOTH)) return BVH_E_INVALID_ARG;
    if (row_capacity >= (1u << 30)) return BVH_E_INVALID_ARG;
    const Range rs[3] = { Range(d_row_first, ((uint64_t)sc->n_inst + 1u) * sizeof(u32)), Range(d_offsets, ((uint64_t)row_capacity + 1u) * sizeof(u32)),
                          fill_range(d_prims, capacity, sizeof(bvh_instance_prim)) };
    if (!disjoint(rs, 3, 3)) return BVH_E_INVALID_ARG;        // the three caller arrays must not overlap
    bvh_ctx* const c = sc->ctx;
    int r;
    // (a one-instance scene on a fresh ctx never made the arena, and rows_word points into it: the smallest one, before the word's address is taken)
    if (!c->arena) { Bind b(c->device); r = ensure_capacity(c, 2); if (r) return r; }
    const SceneCollide rows{ d_row_first, rows_word(c), (flags & BVH_SCENE_COLLIDE_BOTH) ? 1 : 0 };
    if (row_capacity == 0u) {                                 // no rows to answer: the table all the same, d_offsets[0] = total = 0
        Bind b(c->device);
        Install install(c);
        launch_scene_collide_rows(c->stream, scene_query(sc, nullptr, 0, nullptr, nullptr), rows, c->overlap_sums);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(u32), c->stream));
        install.mark();
        if (total_out) *total_out = 0;
        r = 0;
    } else {
        r = count_fill_tail(c, nullptr, row_capacity, d_offsets, total_out, [&](hipStream_t s, u32* overflow, u64* total) {
            SceneQuery q = scene_query(sc, nullptr, row_capacity, d_prims, overflow);
            const SceneHits h{ d_offsets, d_prims, total, capacity };
            launch_scene_collide_rows(s, q, rows, c->overlap_sums);
            launch_scene_collide_count(s, q, h, rows, c->overlap_sums, total);
            if (d_prims) { q.overflow = overflow + 1; launch_scene_collide_fill(s, (flags & BVH_SCENE_COLLIDE_SORTED) ? 1 : 0, q, h, rows); }
        });
        if (r && r != BVH_E_TOO_LARGE) return r;
    }
    if (rows_out) {                                           // the u64 n_rows comes back through total_pairs, as a total does
        Bind b(c->device);
        u32* const rb = total_pairs(c);
        const int w = read_back(c, reinterpret_cast<const u32*>(rows.d_n_rows), 2, nullptr, 0, rb); if (w) return w;
        *rows_out = (uint64_t)rb[0] | ((uint64_t)rb[2] << 32);
        if (*rows_out > row_capacity) return BVH_E_TOO_LARGE;
    }
    return r;
}

// ---- winding numbers on scenes ------------------------------------------------------------------------------------------------------------------
// the scene's winding memory: made by the first prepare after a build (the prefix table from the descriptors' leaf counts, the exchange words all-INVALID)
static int scene_winding_alloc(bvh_scene* sc) {
    const uint32_t n_blas = sc->n_blas;
    std::vector<uint32_t> first(n_blas + 1);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_blas; ++k) { first[k] = (uint32_t)total; total += sc->blas_n[k]; }
    if (total >= (1ull << 32)) return BVH_E_TOO_LARGE;           // (one thread per leaf of all BLASes, 32-bit thread indices)
    first[n_blas] = (uint32_t)total;
    const size_t n = sc->n_inst;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_first = take((n_blas + 1) * sizeof(u32)), o_flags = take(total * sizeof(u32)), o_bmom = take((total - n_blas) * sizeof(bvh_winding_moment));
    const size_t o_maps = take(n * sizeof(bvh_winding_map)), o_imom = take(n * sizeof(bvh_winding_moment)), o_tmom = take(n * sizeof(bvh_winding_moment));
    char* m = nullptr;
    HIP_TRY(hipMalloc(&m, off));
    hipError_t e = hipMemcpy(m + o_first, first.data(), (n_blas + 1) * sizeof(u32), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(m + o_flags, 0xFF, total * sizeof(u32), sc->ctx->stream);
    if (e != hipSuccess) { hipFree(m); return herr(e); }
    sc->wmem = m;
    SceneWind& w = sc->wind;
    w.first = reinterpret_cast<const u32*>(m + o_first); w.flags = reinterpret_cast<u32*>(m + o_flags); w.bmom = reinterpret_cast<bvh_winding_moment*>(m + o_bmom);
    w.maps = reinterpret_cast<bvh_winding_map*>(m + o_maps); w.imom = reinterpret_cast<bvh_winding_moment*>(m + o_imom);
    w.tmom = reinterpret_cast<bvh_winding_moment*>(m + o_tmom);
    w.n_blas = n_blas; w.total_leaves = (uint32_t)total;
    return 0;
}

int bvh_scene_winding_prepare(bvh_scene* sc, uint32_t flags) {
    if (!sc || !sc->built || (flags & ~(uint32_t)BVH_SCENE_WINDING_KEEP_BLAS)) return BVH_E_INVALID_ARG;
    bvh_ctx* c = sc->ctx;
    Bind b(c->device);
    hipStream_t s = c->stream;
    if (!sc->wmem) { const int r = scene_winding_alloc(sc); if (r) return r; }
    Install install(c);
    const bool keep = (flags & BVH_SCENE_WINDING_KEEP_BLAS) && sc->wind_blas_ok;
    sc->wind_ok = false;
    if (!keep) sc->wind_blas_ok = false;
    const SceneQuery q = scene_query(sc, nullptr, 0, nullptr, nullptr);
    if (!keep) launch_scene_winding_blas(s, q, sc->wind);
    launch_scene_winding_top(s, q, sc->wind, sc->flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {                                       // (a refused launch may have left exchange words behind: all-INVALID again before the next climb)
        hipMemsetAsync(sc->wind.flags, 0xFF, (size_t)sc->wind.total_leaves * sizeof(u32), s); hipMemsetAsync(sc->flags, 0xFF, (size_t)sc->n_inst * sizeof(u32), s);
        return herr(e);
    }
    install.mark();
    sc->wind_blas_ok = sc->wind_ok = true;
    return 0;
}

// every argument is checked before anything is enqueued, so an error writes nothing; then bvh_scene_closest_point's tail
int bvh_scene_winding_number(bvh_scene* sc, const bvh_point_query* d_points, uint32_t n_points, float beta, float* d_w) {
    if (!sc || !sc->built || !sc->wind_ok || !d_points || !d_w || !(beta >= 0.0f)) return BVH_E_INVALID_ARG;     // (a NaN beta fails the comparison)
    const Range pts(d_points, (uint64_t)n_points * sizeof(bvh_point_query)), out(d_w, (uint64_t)n_points * sizeof(float));
    if (crosses(pts, out)) return BVH_E_INVALID_ARG;
    if (n_points == 0) return 0;
    return query_tail(sc->ctx, nullptr, sc->overflow, [&](hipStream_t s, u32* overflow) {
        launch_scene_winding(s, scene_query(sc, d_points, n_points, d_w, overflow), sc->wind, beta);
    });
}

int bvh_scene_winding_moments(const bvh_scene* sc, uint32_t blas, const bvh_winding_moment** d_moments, uint32_t* count) {
    if (!sc || !sc->built || !d_moments || !count) return BVH_E_INVALID_ARG;
    if (blas == BVH_INVALID) {
        if (!sc->wind_ok) return BVH_E_INVALID_ARG;
        *d_moments = sc->n_inst >= 2 ? sc->wind.tmom : nullptr; *count = sc->n_inst - 1;
        return 0;
    }
    if (blas >= sc->n_blas || !sc->wind_blas_ok) return BVH_E_INVALID_ARG;
    uint64_t first = 0;
    for (uint32_t k = 0; k < blas; ++k) first += sc->blas_n[k];
    *d_moments = sc->wind.bmom + (first - blas); *count = sc->blas_n[blas] - 1;
    return 0;
}

int bvh_scene_winding_instances(const bvh_scene* sc, const bvh_winding_moment** d_inst_moments, const bvh_winding_map** d_maps) {
    if (!sc || !sc->built || !sc->wind_ok || (!d_inst_moments && !d_maps)) return BVH_E_INVALID_ARG;
    if (d_inst_moments) *d_inst_moments = sc->wind.imom;
    if (d_maps) *d_maps = sc->wind.maps;
    return 0;
}

int bvh_scene_tlas(const bvh_scene* sc, bvh_result* out) {
    if (!sc || !out || !sc->built) return BVH_E_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const uint32_t n = sc->n_inst;
    out->n_leaves = n; out->n_internal = n - 1; out->root = sc->troot; out->layout = sc->tlayout; out->key_bits = 32;
    out->d_prim_aabbs = sc->wbox;
    if (n >= 2) { out->d_nodes = sc->tnodes; out->d_leaves = sc->tlayout == 1 ? sc->tleaves : nullptr; }
    return 0;
}

int bvh_to_lbvh_layout(bvh_ctx* c, const bvh_result* in, void* d_out) {
    if (!c || !in || !d_out || !in->d_nodes) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    if (in->layout == 0) { HIP_TRY(hipMemcpyAsync(d_out, in->d_nodes, (size_t)(2 * in->n_leaves - 1) * sizeof(bvh2_node), hipMemcpyDeviceToDevice, c->stream)); return 0; }
    launch_to_lbvh_layout(c->stream, in->d_nodes, in->d_leaves, in->n_leaves, d_out);
    return herr(hipGetLastError());
}

// CollapseToWide4Bvh + its host set-up (src/TwoPassLbvh.cpp:154-183).  d_bvh4: Bvh4Node[n] (128 B), d_primnodes: PrimNode[n].
int bvh_collapse4(bvh_ctx* c, const bvh_result* in, void* d_bvh4, void* d_primnodes, uint32_t* n_wide_out) {
    if (!c || !in || !in->d_nodes || !d_bvh4 || !d_primnodes) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    const uint32_t n = in->n_leaves;
    int r = ensure_capacity(c, n); if (r) return r;
    hipStream_t s = c->stream;
    uint2* taskq = reinterpret_cast<uint2*>(c->slots);                 // u64[n] scratch, free after a build
    u32* state = c->ploc.state;                                         // >= COLLAPSE_STATE_WORDS words
    static_assert(PLOC_STATE_WORDS >= COLLAPSE_STATE_WORDS, "state scratch");
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev[5], s));
    collapse_begin(s, taskq, state, in->root, true);
    // a batch's level counts come back into pinned words (a copy into pageable memory goes through a staging buffer and blocks); the host polls every one
    // of them (counts are < 2^31: the sentinel is not a count) instead of synchronising the stream — see wait_readback
    u32* const host_pairs = c->h_pinned + 16;
    static_assert(2 * COLLAPSE_MAX_BATCH <= PLOC_STATE_WORDS, "pinned read-back words");
    // wide levels ~ half the BVH2 depth: a first batch sized for a balanced tree — or one above what the previous collapse of a tree of this size needed
    // (animation frames, the benchmark loop: a level launched after the end costs ~3 us) —, then batches of 16 until a level creates nothing
    int batch = 10; for (uint32_t m = n; m > 1u; m >>= 1) batch += 1;
    const uint64_t hint_key = ((uint64_t)in->layout << 32) | (uint64_t)in->root;
    const bool hinted = c->collapse_last_n == n && c->collapse_last_key == hint_key;
    if (hinted && c->collapse_last_levels > 0) batch = (int)c->collapse_last_levels + 1;
    if (batch > COLLAPSE_MAX_BATCH) batch = COLLAPSE_MAX_BATCH;
    u32 base_begin = 0, base_len = 1, levels = 0;                      // the root task
    for (long long total = 0; total < (1ll << 31); total += batch, batch = 16) {
        const bool known = total == 0 && hinted && c->collapse_len_batch > 0 && batch <= c->collapse_len_batch + 1;
        collapse_enqueue(s, in->d_nodes, in->d_leaves, d_bvh4, d_primnodes, taskq, state, base_begin, base_len, batch, n, (int)in->layout,
                         known ? c->collapse_last_len : nullptr);
        HIP_TRY(hipGetLastError());
        r = read_back(c, state, (u32)batch, nullptr, 0, host_pairs); if (r) return r;
        u32 host[COLLAPSE_MAX_BATCH];
        for (int l = 0; l < batch; ++l) host[l] = host_pairs[2 * l];
        u32 len = base_len, allocated = base_begin + base_len;       // ids handed out so far
        u32 lens[COLLAPSE_MAX_BATCH + 1]; lens[0] = base_len;
        for (int l = 0; l < batch; ++l) { if (len) ++levels; len = host[l]; allocated += len; lens[l + 1] = len; }
        if (host[batch - 1] == 0u) {                   // the batch's last level allocated nothing: every later one would have no work
            if (n_wide_out) *n_wide_out = allocated;
            // (remembered only when the whole collapse was one batch: then level l of the next first batch is level l of this one)
            c->collapse_last_n = n; c->collapse_last_levels = levels; c->collapse_last_key = hint_key;
            c->collapse_len_batch = 0;
            if (total == 0) { c->collapse_len_batch = batch; for (int l = 0; l < COLLAPSE_MAX_BATCH; ++l) c->collapse_last_len[l] = l < batch ? lens[l] : 0u; }
            if (c->profiling) {   // token CollapseBvhTime (src/TwoPassLbvh.cpp:182), including this implementation's level read-backs
                HIP_TRY(hipEventRecord(c->ev[6], s)); HIP_TRY(hipEventSynchronize(c->ev[6]));
                HIP_TRY(hipEventElapsedTime(&c->last_collapse_ms, c->ev[5], c->ev[6]));
            }
            return 0;
        }
        base_len = host[batch - 1]; base_begin = allocated - base_len;
        collapse_begin(s, taskq, state, 0u, false);    // clear the counters for the next batch
    }
    return BVH_E_INTERNAL;
}

// GenerateRays (src/CommonBlocksKernel.h:432-463): camera (64-byte Camera record, host pointer) -> Ray[width*height] on the device
int bvh_generate_rays(bvh_ctx* c, const void* h_camera, void* d_rays, uint32_t width, uint32_t height) {
    if (!c || !h_camera || !d_rays || !width || !height) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    HIP_TRY(hipMemcpyAsync(c->small + 16, h_camera, 64, hipMemcpyHostToDevice, c->stream));
    launch_generate_rays(c->stream, c->small + 16, d_rays, width, height);
    return herr(hipGetLastError());
}
// BvhTraversalWhile (src/TraversalKernel.h:238-335) over an LBVH-layout node array; d_rgba (width*height*4 bytes) is cleared first
// (src/TwoPassLbvh.cpp:243: d_colorBuffer.reset()).
int bvh_trace_while(bvh_ctx* c, const void* d_rays, const void* d_tris, const void* d_nodes_lbvh, uint32_t root, uint32_t n_internal,
                    const void* h_transform, void* d_rgba, uint32_t width, uint32_t height) {
    if (!c || !d_rays || !d_tris || !d_nodes_lbvh || !h_transform || !d_rgba || !width || width != height) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    HIP_TRY(hipMemcpyAsync(c->small + 32, h_transform, 64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_rgba, 0, (size_t)width * height * 4, c->stream));
    launch_trace_while(c->stream, d_rays, d_tris, d_nodes_lbvh, c->small + 32, d_rgba, root, width, height, n_internal);
    return herr(hipGetLastError());
}

// the reference's four traversal kernels behind one entry point (src/TraversalKernel.h:49-146, :148-236, :238-335, :337-451)
int bvh_trace(bvh_ctx* c, bvh_trace_kind kind, const void* d_rays, const void* d_tris, const void* d_nodes_lbvh, uint32_t root, uint32_t n_internal,
              const void* h_transform, void* d_rgba, uint32_t* d_ray_counter, uint32_t width, uint32_t height) {
    if (kind == BVH_TRACE_WHILE_WHILE) {
        int r = bvh_trace_while(c, d_rays, d_tris, d_nodes_lbvh, root, n_internal, h_transform, d_rgba, width, height);
        if (r == 0 && d_ray_counter) { Bind b(c->device); HIP_TRY(hipMemsetAsync(d_ray_counter, 0, (size_t)width * height * 4, c->stream)); }   // (that kernel does not count)
        return r;
    }
    if (!c || !d_rays || !d_tris || !d_nodes_lbvh || !h_transform || !d_rgba || !width || width != height) return BVH_E_INVALID_ARG;
    if (kind != BVH_TRACE_RESTART_TRAIL && kind != BVH_TRACE_IF_IF && kind != BVH_TRACE_SPECULATIVE_WHILE) return BVH_E_INVALID_ARG;
    if (kind == BVH_TRACE_RESTART_TRAIL && root != 0) return BVH_E_INVALID_ARG;       // a restart re-enters at node 0 (src/TraversalKernel.h:44)
    Bind b(c->device);
    HIP_TRY(hipMemcpyAsync(c->small + 32, h_transform, 64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_rgba, 0, (size_t)width * height * 4, c->stream));
    launch_trace_kind(c->stream, (int)kind, d_rays, d_tris, d_nodes_lbvh, c->small + 32, d_rgba, d_ray_counter, root, width, height, n_internal);
    return herr(hipGetLastError());
}

int bvh_sah_cost(bvh_ctx* c, const bvh_result* in, double* cost_out) {
    if (!c || !in || !cost_out || !in->d_nodes) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    double* d = reinterpret_cast<double*>(c->small + 8);
    launch_sah_cost(c->stream, in->d_nodes, in->d_leaves, in->root, in->n_leaves, (int)in->layout, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cost_out, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return herr(hipStreamSynchronize(c->stream));
}

int bvh_bvh4_cost(bvh_ctx* c, const void* d_bvh4, uint32_t n_wide, const void* d_primnodes, const void* d_prim_aabbs, uint32_t n, double* cost_out) {
    if (!c || !d_bvh4 || !d_primnodes || !d_prim_aabbs || !cost_out || n < 2 || n_wide == 0 || n_wide > n) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, 2); if (r) return r;
    double* d = reinterpret_cast<double*>(c->small + 8);
    launch_bvh4_cost(c->stream, d_bvh4, n_wide, d_primnodes, d_prim_aabbs, n, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cost_out, d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return herr(hipStreamSynchronize(c->stream));
}

int bvh_checksum(bvh_ctx* c, const bvh_result* in, uint64_t* checksum_out) {
    if (!c || !in || !checksum_out || !in->d_nodes || in->n_leaves < 2) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    int r = ensure_capacity(c, 2); if (r) return r;
    uint64_t* d = reinterpret_cast<uint64_t*>(c->small + 10);
    const uint32_t n = in->n_leaves;
    launch_checksum(c->stream, in->d_nodes, in->layout == 0 ? 2 * n - 1 : n - 1, in->layout == 1 ? in->d_leaves : nullptr, n, in->root, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(checksum_out, d, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    return herr(hipStreamSynchronize(c->stream));
}

int bvh_download(bvh_ctx* c, const bvh_result* in, void* h_nodes, void* h_leaves, void* h_sorted_keys, uint32_t* h_sorted_vals, void* h_scene) {
    if (!c || !in) return BVH_E_INVALID_ARG;
    Bind b(c->device);
    const size_t n = in->n_leaves;
    const size_t node_count = in->layout == 0 ? 2 * n - 1 : n - 1;
    if (h_nodes) HIP_TRY(hipMemcpyAsync(h_nodes, in->d_nodes, node_count * sizeof(bvh2_node), hipMemcpyDeviceToHost, c->stream));
    if (h_leaves && in->d_leaves) HIP_TRY(hipMemcpyAsync(h_leaves, in->d_leaves, n * sizeof(bvh_primref), hipMemcpyDeviceToHost, c->stream));
    if (h_sorted_keys) HIP_TRY(hipMemcpyAsync(h_sorted_keys, in->d_sorted_keys, n * (in->key_bits == 64 ? 8 : 4), hipMemcpyDeviceToHost, c->stream));
    if (h_sorted_vals) HIP_TRY(hipMemcpyAsync(h_sorted_vals, in->d_sorted_vals, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_scene) HIP_TRY(hipMemcpyAsync(h_scene, in->d_scene_extent, sizeof(bvh_aabb), hipMemcpyDeviceToHost, c->stream));
    return herr(hipStreamSynchronize(c->stream));
}

// plain device memory helpers so that non-HIP hosts (ctypes, cgo ...) can stage buffers without linking the HIP runtime
int bvh_dev_alloc(bvh_ctx* c, uint64_t bytes, void** out) { if (!c || !out) return BVH_E_INVALID_ARG; Bind b(c->device); return herr(hipMalloc(out, bytes)); }
int bvh_dev_free(bvh_ctx* c, void* p) { if (!c) return BVH_E_INVALID_ARG; Bind b(c->device); return herr(hipFree(p)); }
int bvh_dev_upload(bvh_ctx* c, void* d_dst, const void* h_src, uint64_t bytes) {
    if (!c) return BVH_E_INVALID_ARG; Bind b(c->device); ++c->tree_serial;
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream)); return herr(hipStreamSynchronize(c->stream)); }
int bvh_dev_download(bvh_ctx* c, void* h_dst, const void* d_src, uint64_t bytes) {
    if (!c) return BVH_E_INVALID_ARG; Bind b(c->device);
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream)); return herr(hipStreamSynchronize(c->stream)); }

int bvh_dev_copy(bvh_ctx* c, void* d_dst, const void* d_src, uint64_t bytes) {   // asynchronous, ordered on the ctx's stream; a kernel, not a runtime copy (misc.hip)
    if (!c || (bytes && (!d_dst || !d_src))) return BVH_E_INVALID_ARG; Bind b(c->device); ++c->tree_serial;
    launch_copy_bytes(c->stream, d_dst, d_src, (size_t)bytes);
    return herr(hipGetLastError()); }

} // extern "C"
