// simplyp_hip.hip -- C ABI (include/simplyp.h) over the gfx950 kernels: context, routing
// schedule, launches.  Built by __graft_entry__.build() into simplyp_amd/csrc/libsimplyp_hip.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <new>
#include <numeric>
#include <string>
#include <variant>
#include <vector>

#include "simplyp_kernels.hip.h"
#include "simplyp_gof.hip.h"
#include "simplyp_gof_lag.hip.h"
#include "simplyp_waterbody.hip.h"
#include "simplyp_quantile.hip.h"
#include "simplyp_order.hip.h"
#include "simplyp_time_quantile.hip.h"
#include "simplyp_predictive.hip.h"
#include "simplyp_forcing.hip.h"
#include "simplyp_score.hip.h"
#include "simplyp_pareto.hip.h"
#include "simplyp_mcmc.hip.h"
#include "simplyp_neldermead.hip.h"
#include "simplyp_nsga2.hip.h"
#include "simplyp_sobol.hip.h"
#include "simplyp_particle.hip.h"
#include "simplyp_pack_stream.h"
#include "simplyp_table.h"
#include "simplyp_weighted.h"
#include "simplyp_score.h"
#include "simplyp_pareto.h"
#include "simplyp_order.h"

namespace {

thread_local std::string g_create_error;

struct DeviceBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
};

}  // namespace

struct simplyp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_start = nullptr, ev_main = nullptr, ev_stop = nullptr;
    hipEvent_t ev_lap[3] = {};          // spare timing events of the analysis entries (generation, sort and contraction laps)
    DeviceBuf route;          // [n_slots][4][D][E] fp64
    DeviceBuf sched;          // int32 schedule arrays
    DeviceBuf counters;       // N_COUNTERS x uint64: rhs, steps, rejected, wave-level attempts, queue waits / longest wait / longest stall
    DeviceBuf balance;        // [E] uint32 pilot counts + [E] int32 permutation
    DeviceBuf sorted_params;  // slot-ordered copies of member_params, reach_params, forcing_of_member
    DeviceBuf forcing_ident;  // opts.forcing_error: [E] int32 identity member -> set map of the generated table
    DeviceBuf gof_lists;      // goodness-of-fit day lists, observations, shifts (simplyp_gof)
    DeviceBuf gof_partial;    // [n_chunks][R][84][E] partial sums
    DeviceBuf quant;          // simplyp_quantiles: 2 x int32 (members used, sweeps) | [E] uint8 include mask in column order
    DeviceBuf wquant;         // simplyp_weighted_quantiles: WqPrepared (T, members used, bad weights, sweeps) | [E] uint64 weights in column order
    DeviceBuf tquant;         // simplyp_time_quantiles: sweeps, rows read | day lists, ranks, output reaches
    DeviceBuf pred;           // simplyp_predictive_*: [R] int32 output reaches (256-byte slot) | a chunk of days [n_series][days][R][E]
    DeviceBuf score;          // simplyp_scores, simplyp_predictive_scores: [E] unit weights | the scored rows' lists | a chunk of rows: sorted pairs twice (, the generated rows)
    DeviceBuf pareto;         // simplyp_pareto: 8 x int32 (n, the peeling's counters) | [E] flags | block offsets | keys [M][E] | 8 x [E] int32 (members, counts, ranks, lists)
    DeviceBuf mcmc;           // simplyp_mcmc_*: 4 x uint32 (inside, accepted, NaN)
    DeviceBuf nm;             // simplyp_nm_*: 8 x uint32 counters
    DeviceBuf nsga2;          // simplyp_nsga2_crowding: keys [M][n] | running keys [4][M][n] (uint64); the counters are `mcmc`'s
    DeviceBuf nm_work;        // simplyp_nm_update: the sort's other copy of the simplexes
    DeviceBuf sobol;          // simplyp_sobol_indices: n_valid | valid [Npad] | mu [n_rows] | n_used [B] | counts [B][Npad] uint16 | sums
    DeviceBuf pf;             // simplyp_pf_*, simplyp_gather_members: PfResult (256-byte slot) | the entry's lists, partial or prefix sums
    DeviceBuf order;          // simplyp_order_members: order_members_device's workspace (a balanced run's own follows its costs in `balance`)
    DeviceBuf queue;          // ticket, error, done[n_groups] (uint32) | ckpt[CKPT_N][E] (double)
    // streamed output (simplyp_stream_out): the armed destination, the chunk flags the queue kernel raises in pinned host
    // memory, and the host thread that turns a raised flag into the D2H copies of that chunk's rows on `copy_stream`
    static constexpr int N_COUNTERS = 8;
    static constexpr int N_COPY_STREAMS = 2;            // measured on C3: 1 stream 803 ms per pass, 2: 795, 3: 796, 4: 799
    hipStream_t copy_stream = nullptr;                  // = copy_streams[0]: carries ev_copy_done
    hipStream_t copy_streams[N_COPY_STREAMS] = {};      // the chunk copies take these in turn
    hipEvent_t ev_copy_done = nullptr, ev_copy_join[N_COPY_STREAMS] = {};
    double* stream_host = nullptr;      // armed for the next run (one-shot)
    int64_t stream_host_bytes = 0;
    const double* state_in = nullptr;   // simplyp_set_state: armed for the next run (one-shot)
    double* state_out = nullptr;
    uint32_t* host_ready = nullptr;     // [host_ready_cap] hipHostMalloc
    size_t host_ready_cap = 0;
    DeviceBuf chunk_count;              // [n_chunks] uint32
    struct CopyPlan {                   // what a run decides of its streamed copy
        const double* dev = nullptr;
        double* host = nullptr;
        bool chunked = false;           // chunk by chunk beside the queue kernel (`table` says which), not the whole table behind the run
        simplyp_pack::Table table = {}; // columns, days, doubles per row (n_out_reaches * E), time chunks; the records' geometry
        const unsigned char* pack_dev = nullptr;    // the packed records (simplyp_pack.h); null: every chunk travels as fp64
    } copy_plan;
    simplyp_pack::Tally tally;          // what the copier sent packed and raw
    DeviceBuf packed;                   // the packed records of a run (grow-only; given back by the first run that does not pack)
    DeviceBuf pack_count;               // [n_records][2] uint32: overflow blocks, body words; then [n_cols] int32: Table::pred
    uint32_t* host_pack_count = nullptr;    // the same in pinned host memory, written by the wave that completes a chunk
    size_t host_pack_count_cap = 0;
    simplyp_pack::PackStream pack;      // staging ring, dispatcher and decode pool
    std::thread copier;
    std::atomic<int> run_over{0};       // set by simplyp_sync once the launches have finished (the copier stops waiting for flags)
    int copy_error = 0;                 // first hipError_t the copier saw
    int streamed_chunks = 0;            // chunks whose copy started before the kernel had finished
    bool copy_pending = false;
    std::chrono::steady_clock::time_point t_begin;
    int n_simd_slots = 1024;  // CUs x 4 SIMDs: wave slots at one resident wave per SIMD
    simplyp_stats last = {};  // what the shape of the last run decides of its stats (simplyp_sync adds the measurements)
    bool pending = false;
    std::string error;
};

namespace {

int fail(simplyp_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->error = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, call)                                                                         \
    do {                                                                                           \
        hipError_t err__ = (call);                                                                 \
        if (err__ != hipSuccess)                                                                   \
            return fail(ctx, SIMPLYP_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(err__)); \
    } while (0)

int ensure(simplyp_ctx* ctx, DeviceBuf& b, size_t bytes)
{
    if (bytes <= b.bytes) return SIMPLYP_OK;
    if (b.ptr) { (void)hipFree(b.ptr); b.ptr = nullptr; b.bytes = 0; }
    hipError_t err = hipMalloc(&b.ptr, bytes);
    if (err != hipSuccess)
        return fail(ctx, SIMPLYP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(err));
    b.bytes = bytes;
    return SIMPLYP_OK;
}

// Host-side C++ (std::vector, std::thread) must not throw across the C boundary: every exported function that allocates
// runs its body through this.
template <class F>
int guarded(simplyp_ctx* ctx, F&& body)
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(ctx, SIMPLYP_ERR_NOMEM, "host memory allocation failed");
    } catch (const std::exception& e) {
        return fail(ctx, SIMPLYP_ERR_DEVICE, "unexpected host error: %s", e.what());
    }
}

// ceil(n / threads): the blocks of a one-dimensional grid.
template <class N>
unsigned blocks(N n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// A 64-bit seed as the two halves of a Philox key.
template <class G>
void philox_key(uint64_t seed, G& g)
{
    g.key0 = (uint32_t)(seed & 0xFFFFFFFFull);
    g.key1 = (uint32_t)(seed >> 32);
}

// One launch = a set of mutually independent chains; a chain = reaches one thread walks in order.
struct Launch {
    std::vector<int> chain_ptr;     // n_chains + 1, offsets into chain_reach
    std::vector<int> chain_reach;
};

struct Schedule {
    std::vector<Launch> launches;
    std::vector<int> route_slot;    // [S], -1 when nobody reads the reach's series
    int n_slots = 0;
};

// Routing schedule from the upstream CSR (reference: SC loop in ascending id, model.py:365, each
// reach reading its upstream reaches' finished series, :521-528).  Reaches whose upstream reaches
// are all done form a launch; a reach's single downstream reach is appended to the same chain
// (processed by the same thread, "sequential chain inside the kernel") when nothing else feeds it
// that is not already done.  Series slots are recycled as soon as every reader has finished;
// inside a chain the slots alternate, since element k+1 is the only reader of element k.
int build_schedule(simplyp_ctx* ctx, int S, const int32_t* up_ptr, const int32_t* up_idx, Schedule& sch)
{
    std::vector<std::vector<int>> down(S);
    for (int s = 0; s < S; ++s) {
        if (up_ptr[s + 1] < up_ptr[s]) return fail(ctx, SIMPLYP_ERR_TOPOLOGY, "up_ptr not monotone at reach %d", s);
        for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) {
            const int u = up_idx[k];
            if (u < 0 || u >= s)
                return fail(ctx, SIMPLYP_ERR_TOPOLOGY, "reach %d lists upstream reach %d (must be in [0, %d))", s, u, s);
            down[u].push_back(s);
        }
    }
    sch.route_slot.assign(S, -1);
    std::vector<char> done(S, 0), taken(S, 0);
    std::vector<int> readers_left(S, 0);
    for (int s = 0; s < S; ++s) readers_left[s] = (int)down[s].size();
    std::vector<int> free_slots;
    int n_done = 0;
    auto alloc_slot = [&]() {
        if (!free_slots.empty()) { int v = free_slots.back(); free_slots.pop_back(); return v; }
        return sch.n_slots++;
    };
    while (n_done < S) {
        Launch L;
        L.chain_ptr.push_back(0);
        for (int s = 0; s < S; ++s) {
            if (done[s] || taken[s]) continue;
            bool ready = true;
            for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) ready = ready && done[up_idx[k]];
            if (!ready) continue;
            int cur = s;
            taken[cur] = 1;
            L.chain_reach.push_back(cur);
            for (;;) {
                if (down[cur].size() != 1) break;
                const int dn = down[cur][0];
                if (taken[dn] || done[dn]) break;
                bool ok = true;
                for (int k = up_ptr[dn]; k < up_ptr[dn + 1]; ++k)
                    ok = ok && (up_idx[k] == cur || done[up_idx[k]]);
                if (!ok) break;
                taken[dn] = 1;
                L.chain_reach.push_back(dn);
                cur = dn;
            }
            L.chain_ptr.push_back((int)L.chain_reach.size());
        }
        if (L.chain_reach.empty()) return fail(ctx, SIMPLYP_ERR_TOPOLOGY, "reach graph has no schedulable reach");
        // Series slots.  A slot is column-partitioned by member, and a chain is walked by one thread per
        // member, so a slot released inside a chain (its only reader was the next element) may be reused
        // by later elements of the SAME chain at once; every other release waits for the launch to end.
        std::vector<int> pending;
        for (size_t c = 0; c + 1 < L.chain_ptr.size(); ++c) {
            std::vector<int> local_free;
            int prev = -1;
            for (int i = L.chain_ptr[c]; i < L.chain_ptr[c + 1]; ++i) {
                const int s = L.chain_reach[i];
                if (!down[s].empty()) {
                    if (!local_free.empty()) { sch.route_slot[s] = local_free.back(); local_free.pop_back(); }
                    else sch.route_slot[s] = alloc_slot();
                }
                for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) {
                    const int u = up_idx[k];
                    if (--readers_left[u] == 0 && sch.route_slot[u] >= 0)
                        (u == prev ? local_free : pending).push_back(sch.route_slot[u]);
                }
                prev = s;
            }
            pending.insert(pending.end(), local_free.begin(), local_free.end());
        }
        free_slots.insert(free_slots.end(), pending.begin(), pending.end());
        for (int s : L.chain_reach) { done[s] = 1; ++n_done; }
        sch.launches.push_back(std::move(L));
    }
    return SIMPLYP_OK;
}

int popcount32(uint32_t v) { return __builtin_popcount(v); }

using simplyp_order::order_members;       // the host rule (simplyp_order.h)

// order_members' rule on the device (simplyp_order.hip.h): d_cost -> d_perm on the run's stream, nothing copied and nothing
// waited for.  The workspace follows d_perm in ctx->balance (order_workspace_bytes).
bool order_on_device(int E)
{
    const char* env = getenv("SIMPLYP_ORDER_HOST");           // read at every run: 1 = the host's order_members
    return !(env && atoi(env) == 1) && E <= simplyp::ORD_MAX_E;
}

int order_sort_keys(int E)
{
    int P = simplyp::ORD_CHUNK;
    while (P < E) P <<= 1;
    return P;
}

size_t order_workspace_bytes(int E)
{
    const size_t n_groups = ((size_t)E + simplyp::ORD_THREADS - 1) / simplyp::ORD_THREADS;
    return 8 + (size_t)order_sort_keys(E) * sizeof(unsigned long long) +
           (n_groups * (2 * simplyp::ORD_WIN + simplyp::ORD_NCOV) + 2 * simplyp::ORD_WIN) * sizeof(double) + 2 * simplyp::ORD_WIN * sizeof(float);
}

int order_members_device(simplyp_ctx* ctx, const uint32_t* d_cost, int32_t* d_perm, void* work, int E)
{
    namespace sp = simplyp;
    sp::OrderArgs g;
    g.E = E;
    g.P = order_sort_keys(E);
    g.n_groups = (E + sp::ORD_THREADS - 1) / sp::ORD_THREADS;
    g.nb1 = std::max(1, std::min(sp::ORD_MAX_BLOCKS, E / sp::ORD_MIN_BLOCK));
    g.nb2 = std::max(1, std::min(sp::ORD_MAX_SUB, E / (g.nb1 * sp::ORD_MIN_BLOCK)));
    g.cost = d_cost;
    g.key = (unsigned long long*)(((uintptr_t)work + 7) & ~(uintptr_t)7);
    g.part_stats = (double*)(g.key + g.P);
    g.part_cov = g.part_stats + (size_t)g.n_groups * 2 * sp::ORD_WIN;
    g.moments = g.part_cov + (size_t)g.n_groups * sp::ORD_NCOV;
    g.vec = (float*)(g.moments + 2 * sp::ORD_WIN);
    g.perm = d_perm;
    const dim3 wg(sp::ORD_THREADS);
    hipLaunchKernelGGL(sp::order_stats_kernel, dim3((unsigned)(g.P / sp::ORD_THREADS)), wg, 0, ctx->stream, g);
    hipLaunchKernelGGL(sp::order_cov_kernel, dim3((unsigned)g.n_groups), wg, 0, ctx->stream, g);
    hipLaunchKernelGGL(sp::order_pca_kernel, dim3(1), dim3(64), 0, ctx->stream, g);
    const dim3 chunks((unsigned)(g.P / sp::ORD_CHUNK));
    hipLaunchKernelGGL(sp::order_sort_chunk_kernel, chunks, wg, 0, ctx->stream, g.key, 2);
    for (int k = 2 * sp::ORD_CHUNK; k <= g.P; k <<= 1) {
        for (int j = k >> 1; j >= sp::ORD_CHUNK; j >>= 1)
            hipLaunchKernelGGL(sp::order_sort_stride_kernel, dim3((unsigned)(g.P / 2 / 256)), dim3(256), 0, ctx->stream, g.key, g.P, k, j);
        hipLaunchKernelGGL(sp::order_sort_chunk_kernel, chunks, wg, 0, ctx->stream, g.key, k);
    }
    hipLaunchKernelGGL(sp::order_blocks_kernel, dim3((unsigned)g.nb1), wg, 0, ctx->stream, g);
    HIP_TRY(ctx, hipGetLastError());
    return SIMPLYP_OK;
}

// Host side of the streamed output: wait for the kernel to raise a chunk's flag (or for the run to be over), then enqueue the
// chunk's rows of every column on the copy stream.  Rows of one chunk are contiguous inside a column of `out`
// ([col][day][reach][member]), so a chunk is `ncols` plain copies.
void copier_main(simplyp_ctx* ctx)
{
    (void)hipSetDevice(ctx->device);
    const simplyp_ctx::CopyPlan& p = ctx->copy_plan;
    const simplyp_pack::Table& t = p.table;
    // No HIP call inside the wait: hipEventQuery on the run's stop event blocks for as long as another thread sits in
    // hipEventSynchronize on it (measured: the first query returned when the kernel ended).  The flags live in host memory;
    // "the run is over" comes from simplyp_sync (or the error paths) through `run_over`.
    bool run_over = false;
    unsigned n_issued = 0;
    const bool dbg = getenv("SIMPLYP_DEBUG") != nullptr;
    auto note = [&](hipError_t err) { if (err != hipSuccess && !ctx->copy_error) ctx->copy_error = (int)err; };
    // two streams, taken in turn: the launch gap of one copy dispatch hides behind the other stream's transfer
    auto next_stream = [&] { return ctx->copy_streams[n_issued++ % (unsigned)simplyp_ctx::N_COPY_STREAMS]; };
    // (one plain copy per column: a pitched hipMemcpy2DAsync per chunk does not overlap the persistent kernel at all on this
    // stack -- 1509 ms per pass instead of 803, profiles/r02_experiments.md)
    auto raw = [&](size_t off, size_t bytes) { note(hipMemcpyAsync(p.host + off, p.dev + off, bytes, hipMemcpyDeviceToHost, next_stream())); };
    // every finished chunk travels at once: one copy per column (51 MB for C3).  Several chunks per copy were tried against the
    // spells at 45-50 instead of 56 GB/s this pool sometimes has, and changed nothing (profiles/r02_experiments.md)
    for (int c = 0; c < t.n_chunks(); ++c) {
        while (!run_over && __atomic_load_n(&ctx->host_ready[c], __ATOMIC_ACQUIRE) == 0u) {
            if (ctx->run_over.load(std::memory_order_acquire)) { run_over = true; break; }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        if (!run_over) ++ctx->streamed_chunks;
        if (dbg && (c < 3 || c + 2 > t.n_chunks()))
            fprintf(stderr, "[simplyp] copier: chunk %d ready=%u over=%d at %.1f ms\n", c, ctx->host_ready[c], (int)run_over,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->t_begin).count());
        // a chunk whose flag never rose (the run ended in an error) has no valid counters: it travels raw
        if (!p.pack_dev || __atomic_load_n(&ctx->host_ready[c], __ATOMIC_ACQUIRE) == 0u) {
            for (int j = 0; j < t.n_cols; ++j) raw(t.offset(j, c), t.raw_bytes(c));
            continue;
        }
        // the records instead of the rows: into the staging ring, and from there through the decode pool into p.host
        const uint32_t* count = ctx->host_pack_count + 2 * t.record(c, 0);
        simplyp_pack::route_chunk(t, c, p.pack_dev, p.host, ctx->tally,
                                  [&](int j, unsigned& overflow_blocks, size_t& words) { overflow_blocks = count[2 * j]; words = count[2 * j + 1]; },
                                  [&](const simplyp_pack::PackJob& job) { note(ctx->pack.submit(job, next_stream())); }, raw);
    }
    hipError_t err = hipSuccess;
    for (int i = 1; i < simplyp_ctx::N_COPY_STREAMS && err == hipSuccess; ++i) {        // stream 0 joins the others, then signals
        err = hipEventRecord(ctx->ev_copy_join[i], ctx->copy_streams[i]);
        if (err == hipSuccess) err = hipStreamWaitEvent(ctx->copy_stream, ctx->ev_copy_join[i], 0);
    }
    if (err == hipSuccess) err = hipEventRecord(ctx->ev_copy_done, ctx->copy_stream);
    note(err);
}

int check_args(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts, const void* forcing, const int32_t* doy,
               const int32_t* period_of_day, const void* mp, const void* rp, const int32_t* up_ptr, const int32_t* up_idx,
               const void* out, const void* status, const int32_t* member_of_slot, const int32_t* out_reaches,
               int32_t n_out_reaches, const double* host_out, int64_t host_out_bytes)
{
    if (!dims || !opts) return fail(ctx, SIMPLYP_ERR_ARG, "dims/opts is NULL");
    if (dims->E <= 0 || dims->S <= 0 || dims->D <= 0 || dims->n_forcing_sets <= 0)
        return fail(ctx, SIMPLYP_ERR_ARG, "bad dims E=%d S=%d D=%d n_forcing_sets=%d", dims->E, dims->S, dims->D,
                    dims->n_forcing_sets);
    if (!forcing || !mp || !rp || !up_ptr || !out || !status)
        return fail(ctx, SIMPLYP_ERR_ARG, "a required pointer is NULL");
    if (opts->integrator != SIMPLYP_INTEG_RK4 && opts->integrator != SIMPLYP_INTEG_CASHKARP &&
        opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG && opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG_F32)
        return fail(ctx, SIMPLYP_ERR_ARG, "unknown integrator %d", opts->integrator);
    if (opts->integrator == SIMPLYP_INTEG_RK4 && opts->substeps <= 0)
        return fail(ctx, SIMPLYP_ERR_ARG, "RK4 needs substeps >= 1 (got %d)", opts->substeps);
    if (opts->integrator != SIMPLYP_INTEG_RK4 && (!(opts->rtol > 0.0) || !(opts->atol >= 0.0) || opts->max_steps < 1))
        return fail(ctx, SIMPLYP_ERR_ARG, "Cash-Karp needs rtol > 0, atol >= 0, max_steps >= 1");
    if (opts->integrator == SIMPLYP_INTEG_CASHKARP_AUG_F32 && opts->rtol < 1e-6)
        return fail(ctx, SIMPLYP_ERR_ARG, "fp32 stages cannot resolve rtol < 1e-6 (got %g): use integrator 2", opts->rtol);
    if (opts->lanes_per_member != 0 && opts->lanes_per_member != 1 && opts->lanes_per_member != 4)
        return fail(ctx, SIMPLYP_ERR_ARG, "lanes_per_member must be 0 (auto), 1 or 4 (got %d)", opts->lanes_per_member);
    if (opts->lanes_per_member == 4 && opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG)
        return fail(ctx, SIMPLYP_ERR_ARG, "lanes_per_member = 4 exists for integrator 2 (Cash-Karp on the augmented system) only");
    if (opts->stiff_pair > 0 && opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG)
        return fail(ctx, SIMPLYP_ERR_ARG, "stiff_pair > 0 (the stability-optimised second pair) exists for integrator 2 (Cash-Karp on the augmented system) only");
    if (!(opts->step_len > 0.0) || !std::isfinite(opts->step_len))
        return fail(ctx, SIMPLYP_ERR_ARG, "step_len must be finite and > 0 (got %g)", opts->step_len);
    if (opts->sc_qr0 < 0 || opts->sc_qr0 >= dims->S) return fail(ctx, SIMPLYP_ERR_ARG, "sc_qr0 out of range");
    if (opts->out_mask == 0u || (opts->out_mask & ~(SIMPLYP_MASK_ALL | SIMPLYP_MASK_D_SNOW)) != 0u)
        return fail(ctx, SIMPLYP_ERR_ARG, "out_mask must select 1..%d of the columns", (int)SIMPLYP_N_OUT);
    if ((opts->out_mask & SIMPLYP_MASK_D_SNOW) != 0u && !opts->snow)
        return fail(ctx, SIMPLYP_ERR_ARG, "column D_snow (SIMPLYP_OUT_D_SNOW) exists only when the snow module runs in the kernel (opts.snow = 1)");
    if (out_reaches) {
        if (n_out_reaches <= 0 || n_out_reaches > dims->S) return fail(ctx, SIMPLYP_ERR_ARG, "bad n_out_reaches");
        for (int k = 0; k < n_out_reaches; ++k)
            if (out_reaches[k] < 0 || out_reaches[k] >= dims->S) return fail(ctx, SIMPLYP_ERR_ARG, "out_reaches[%d] out of range", k);
    }
    if (host_out && host_out_bytes < simplyp_out_bytes(dims, opts, out_reaches ? n_out_reaches : dims->S))
        return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_stream_out: host buffer of %lld bytes is smaller than the output table (%lld)",
                    (long long)host_out_bytes, (long long)simplyp_out_bytes(dims, opts, out_reaches ? n_out_reaches : dims->S));
    if (opts->dynamic_erod && !doy) return fail(ctx, SIMPLYP_ERR_ARG, "doy is required when dynamic_erod is set");
    if (opts->n_periods < 0 || (opts->n_periods > 0 && !period_of_day))
        return fail(ctx, SIMPLYP_ERR_ARG, "n_periods > 0 needs period_of_day (and n_periods must not be negative)");
    if (opts->out_slot_order && !member_of_slot)
        return fail(ctx, SIMPLYP_ERR_ARG, "out_slot_order = 1 needs member_of_slot");
    if (up_ptr[dims->S] > 0 && !up_idx) return fail(ctx, SIMPLYP_ERR_ARG, "up_idx is NULL but up_ptr lists upstream reaches");
    if (opts->forcing_error) {
        static const char* const row_name[3] = {"P", "PET", "T_air"};
        if (!opts->forcing_table)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_error needs forcing_table: the device workspace [E][%d][D] the members' forcing is written to",
                        opts->snow ? 3 : 2);
        for (int r = 0; r < 3; ++r) {
            const double sg = opts->forcing_sigma[r];
            if (!std::isfinite(sg) || sg < 0.0 || sg > 2.0)
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_sigma[%d] (%s) must be finite and in [0, 2] (got %g)", r, row_name[r], sg);
            if (sg > 0.0 && !opts->forcing_group_of_day[r])
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_sigma[%d] (%s) > 0 needs forcing_group_of_day[%d]: the group id of every day", r,
                            row_name[r], r);
        }
        if (opts->forcing_sigma[2] > 0.0 && !opts->snow)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_sigma[2] > 0 perturbs T_air, a forcing row only with the snow module in the kernel (opts.snow = 1)");
        if (opts->forcing_shift ? (opts->forcing_shift_rows != 2 && opts->forcing_shift_rows != 3) : opts->forcing_shift_rows != 0)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_shift_rows must be 2 or 3 with forcing_shift and 0 without (got %d)", opts->forcing_shift_rows);
        if ((long long)dims->E * ((dims->D + simplyp::FORCING_THREADS - 1) / simplyp::FORCING_THREADS) > 0x7fffffffLL)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_error: E x ceil(D / %d) must stay below 2^31", simplyp::FORCING_THREADS);
        if (opts->forcing_shift_rows == 3 && !opts->snow)
            return fail(ctx, SIMPLYP_ERR_ARG, "a T_air offset (forcing_shift_rows = 3) needs the snow module in the kernel (opts.snow = 1)");
        bool any_rho = false;
        for (int r = 0; r < 3; ++r) {
            const double rho = opts->forcing_rho[r];
            if (!std::isfinite(rho) || rho < 0.0 || rho > 0.999)
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_rho[%d] (%s) must be finite and in [0, 0.999] (got %g)", r, row_name[r], rho);
            if (rho > 0.0 && !(opts->forcing_sigma[r] > 0.0))
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_rho[%d] (%s) > 0 needs forcing_sigma[%d] > 0: there is no error to correlate", r,
                            row_name[r], r);
            any_rho = any_rho || rho > 0.0;
        }
        if (!any_rho && (opts->forcing_noise_in || opts->forcing_noise_out))
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_noise_in / forcing_noise_out need some forcing_rho > 0: without one no noise state exists");
        if (any_rho && (long long)dims->E * (opts->snow ? 3 : 2) > 0x7fffffffLL)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_rho: E x rows must stay below 2^31");
        const int G = opts->forcing_shift_groups;
        if (G < 0 || G > 4096)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_shift_groups must be 0 or in [1, 4096] (got %d)", G);
        if (G >= 1 && (!opts->forcing_shift_group_of_day || !opts->forcing_shift))
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_shift_groups = %d needs forcing_shift_group_of_day and forcing_shift [rows][%d][E]", G, G);
        if (G == 0 && opts->forcing_shift_group_of_day)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_shift_group_of_day needs forcing_shift_groups >= 1: the number of shift groups");
        if (opts->forcing_reserved2)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_reserved2 must be 0");
        if (opts->forcing_pet_model != 0 && opts->forcing_pet_model != 1)
            return fail(ctx, SIMPLYP_ERR_ARG, "forcing_pet_model must be 0 (off) or 1 (Thornthwaite) (got %d)", opts->forcing_pet_model);
        if (opts->forcing_pet_model) {
            if (!opts->snow)
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_pet_model = 1 derives PET from the member's T_air row, a forcing row only with the snow module in the kernel (opts.snow = 1)");
            const int years = dims->D / 365;                                   // whole calendar years: 365 each and the leap days
            if (years < 1 || dims->D - 365 * years > years / 4 + 1)
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_pet_model = 1 needs whole calendar years of daily values: D = %d is no 365 x years + leap days", dims->D);
            if (years > SIMPLYP_FORCING_PET_YEARS_MAX)
                return fail(ctx, SIMPLYP_ERR_ARG, "forcing_pet_model = 1 takes at most %d years: the monthly values of a member live in LDS (D = %d is %d)",
                            (int)SIMPLYP_FORCING_PET_YEARS_MAX, dims->D, years);
        }
    } else if (opts->forcing_pet_model) {
        return fail(ctx, SIMPLYP_ERR_ARG, "forcing_pet_model needs forcing_error = 1");
    } else if (opts->forcing_rho[0] != 0.0 || opts->forcing_rho[1] != 0.0 || opts->forcing_rho[2] != 0.0 || opts->forcing_noise_in ||
               opts->forcing_noise_out || opts->forcing_shift_group_of_day || opts->forcing_shift_groups) {
        return fail(ctx, SIMPLYP_ERR_ARG, "forcing_rho, forcing_noise_in / _out, forcing_shift_group_of_day and forcing_shift_groups need forcing_error = 1");
    }
    return SIMPLYP_OK;
}

// opts.forcing_error: writes every member's forcing set into opts.forcing_table and the identity member -> set map into the
// context's scratch, on the run's stream; `a` then reads the table as E forcing sets.
int generate_forcing(simplyp_ctx* ctx, const simplyp_opts& opts, simplyp::KernelArgs& a)
{
    if (int rc = ensure(ctx, ctx->forcing_ident, (size_t)a.E * sizeof(int32_t))) return rc;
    simplyp::ForcingErrorArgs g{};
    g.E = a.E; g.D = a.D; g.rows = opts.snow ? 3 : 2;
    g.day_blocks = (a.D + simplyp::FORCING_THREADS - 1) / simplyp::FORCING_THREADS;
    g.base = a.forcing; g.forcing_of_member = a.forcing_of_member;
    for (int r = 0; r < 3; ++r) {
        g.sigma[r] = r < g.rows ? opts.forcing_sigma[r] : 0.0;
        g.group[r] = g.sigma[r] > 0.0 ? opts.forcing_group_of_day[r] : nullptr;
    }
    g.shift = opts.forcing_shift; g.shift_rows = opts.forcing_shift ? opts.forcing_shift_rows : 0;
    g.shift_groups = opts.forcing_shift_groups; g.shift_group = opts.forcing_shift_group_of_day;
    bool ar1 = false;
    for (int r = 0; r < g.rows; ++r) {
        g.rho[r] = opts.forcing_rho[r];
        g.c[r] = std::sqrt(1.0 - g.rho[r] * g.rho[r]);
        ar1 = ar1 || g.rho[r] > 0.0;
    }
    g.noise_in = opts.forcing_noise_in; g.noise_out = opts.forcing_noise_out;
    g.key0 = (uint32_t)(opts.forcing_seed & 0xffffffffu); g.key1 = (uint32_t)(opts.forcing_seed >> 32);
    g.member0 = opts.forcing_member0;
    g.table = opts.forcing_table; g.ident = (int32_t*)ctx->forcing_ident.ptr;
    g.pet_model = opts.forcing_pet_model;
    if (ar1) {                                                            // one wave per (member, row)
        const long long waves = (long long)a.E * g.rows;                  // (check_args: below 2^31)
        const unsigned blocks = (unsigned)((waves + simplyp::FORCING_AR1_WAVES - 1) / simplyp::FORCING_AR1_WAVES);
        hipLaunchKernelGGL(simplyp::simplyp_forcing_ar1_kernel, dim3(blocks), dim3(simplyp::FORCING_THREADS), 0, ctx->stream, g);
    } else {
        const unsigned blocks = (unsigned)a.E * (unsigned)g.day_blocks;   // (check_args: fits the grid)
        hipLaunchKernelGGL(simplyp::simplyp_forcing_error_kernel, dim3(blocks), dim3(simplyp::FORCING_THREADS), 0, ctx->stream, g);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (opts.forcing_pet_model) {                                         // PET from the T_air row just written, one block per member
        simplyp::ForcingPetArgs p{};
        p.E = a.E; p.D = a.D; p.Y = a.D / 365; p.M = 12 * p.Y;                // (check_args: snow, whole years, Y <= cap)
        p.daylight = opts.forcing_table + (size_t)a.E * 3 * (size_t)a.D;     // the plan behind the table: daylight[M], month[2][M], day[3][D]
        p.month = (const int32_t*)(p.daylight + p.M);
        p.day = p.month + 2 * p.M;
        p.table = opts.forcing_table;
        p.has_f = g.sigma[1] > 0.0 || g.shift_rows >= 2;
        hipLaunchKernelGGL(simplyp::simplyp_forcing_pet_kernel, dim3((unsigned)a.E), dim3(simplyp::PET_THREADS), 0, ctx->stream, p);
        HIP_TRY(ctx, hipGetLastError());
    }
    a.forcing = opts.forcing_table; a.n_sets = a.E; a.forcing_of_member = g.ident;
    return SIMPLYP_OK;
}

// The shape of a run: how members map to lanes and waves, which pair and kernel run it, how it cuts time and whether a pilot
// balances it first.  Decided from the arguments, the chip's wave slots and whether a streamed output is armed; no HIP call.
struct RunShape {
    int team = 1;                  // lanes per member: 1, or 4 = one member per DPP quad
    int lanes = simplyp::WAVE;     // member slots per wavefront
    unsigned gx = 0;               // member groups: waves per chain
    bool stiff = false;            // integrator 2 with the stability-optimised second pair
    bool stream_chunks = false;    // a streamed output wants the table in time chunks
    int chunk_days = 0, n_chunks = 0;
    bool want_queue = false;       // the task-queue kernel as wanted (launch_queue falls back to the chain kernel if it does not fit)
    int pilot_days = 0;
    bool balance = false;          // a pilot run orders the members by cost
};

RunShape plan_run(const simplyp_dims& dims, const simplyp_opts& opts, int n_simd_slots, bool streamed)
{
    const int E = dims.E, S = dims.S, D = dims.D;
    RunShape r;
    // Member slots per wavefront.  64 unless the ensemble cannot fill the chip with full waves: a single-reach ensemble under an
    // adaptive integrator is then spread over as many waves as there are SIMDs (a wave's day costs its slowest lane's attempts;
    // idle SIMDs cost nothing).  Results do not depend on it (members are independent).
    // Lanes per member: 1, or 4 -- a member's Cash-Karp attempt spread over a DPP quad (ck_day_quad: ~1.4 x shorter attempts,
    // bit-identical results) -- when the ensemble is so small that even then every (member group, reach) finds a resident wave
    // of its own: the run is bound by one member's serial chain of attempts, not by throughput.  A single-reach ensemble may be
    // up to 1.75 x larger than that: its quads then run through the work-conserving task queue in ~1.5 rounds of waves that all
    // SIMDs share, where the one-lane kernel would keep a third of the SIMDs busy for one long round (measured, MI355X:
    // 25 000 members 477 against 598 ms, 30 000 members 571 against 600, 40 000 members 759 against 610).
    const long long quad_waves = (long long)((E + 15) / 16) * S;
    if (opts.integrator == SIMPLYP_INTEG_CASHKARP_AUG &&
        (opts.lanes_per_member == 4 ||
         (opts.lanes_per_member == 0 && (quad_waves <= (long long)n_simd_slots ||
                                         (S == 1 && quad_waves * 4 <= 7LL * n_simd_slots)))))
        r.team = 4;
    const int max_lanes = simplyp::WAVE / r.team;
    r.lanes = max_lanes;
    if (opts.lanes_per_wave > 0) r.lanes = std::min<int>(max_lanes, opts.lanes_per_wave);
    else if (opts.integrator != SIMPLYP_INTEG_RK4 && S == 1 && (E + max_lanes - 1) / max_lanes < n_simd_slots)
        r.lanes = std::max(1, (E + n_simd_slots - 1) / n_simd_slots);
    r.gx = (unsigned)((E + r.lanes - 1) / r.lanes);
    // opts.stiff_pair (integrator 2): attempts bound by Cash-Karp's stability interval go to the second pair; auto = reach networks
    r.stiff = opts.integrator == SIMPLYP_INTEG_CASHKARP_AUG && SIMPLYP_STIFF_PAIR_ON(opts.stiff_pair, S);
    // (a streamed output wants time chunks: their rows travel to the host while later chunks compute -- and short ones, so that
    // the first copy starts early: the copies, not the kernel, bound a streamed pass; 64 days cost ~0.4 % in task overhead)
    r.stream_chunks = streamed && opts.n_periods == 0;
    r.chunk_days = opts.time_chunk_days > 0 ? opts.time_chunk_days : ((r.stream_chunks && S == 1) ? 64 : 256);
    r.chunk_days = ((r.chunk_days + 63) / 64) * 64;
    r.n_chunks = (D + r.chunk_days - 1) / r.chunk_days;
    // task-queue kernel, auto: when the chain kernel would leave SIMDs idle -- a single-reach ensemble that needs more waves than
    // the chip holds at once, or a multi-reach network (a chain walked by one thread per member cannot use more than E lanes)
    r.want_queue = opts.integrator != SIMPLYP_INTEG_RK4 && D > r.chunk_days &&
        (opts.time_chunk_days > 0 || (r.stream_chunks && opts.time_chunk_days == 0) ||
         (opts.time_chunk_days == 0 && ((S == 1 && (int)r.gx > n_simd_slots) || (S > 1 && (int)r.gx < n_simd_slots))));
    // Load balance (Cash-Karp only: members differ in the steps they need).
    // With more waves than the chip holds at once, the run takes as long as the unluckiest SIMD's queue.
    // A short pilot run measures each member's cost; members are then handed to lane slots in order of
    // decreasing cost, so (a) the lanes of a wave need similar step counts and (b) the dispatcher starts
    // the long waves first and back-fills with the short ones (longest-processing-time-first).
    r.pilot_days = opts.balance_pilot_days > 0 ? opts.balance_pilot_days : 64;
    if (r.pilot_days > D) r.pilot_days = D;
    // auto: a single-reach ensemble that needs more waves than the chip holds at once; a reach network that will run through
    // the task queue with at least four member groups (there every SIMD works through many tasks, so homogeneous groups pay;
    // with one wave per SIMD sorting only makes the slowest wave slower).  It reads the queue as wanted: a queue that does not
    // fit and falls back to the chain kernel leaves the decision as it is.
    r.balance = opts.integrator != SIMPLYP_INTEG_RK4 && r.pilot_days * 4 <= D &&
        (opts.balance == 1 ||
         (opts.balance == 2 && ((int)r.gx > n_simd_slots || (S > 1 && r.want_queue && r.gx >= 4u))));
    return r;
}

// Pilot launches of the load balancer on a reach network: the routing schedule cut off PILOT_LEVELS reaches below the
// headwaters (chains keep their first elements; the slot assignments of the full schedule stay valid for a subset run
// in the same order).  Every reach of a member shares the member's parameters, so its cost rank among the members
// carries over to the reaches further down; a 256-reach chain is sampled by its first 8 reaches.
constexpr int PILOT_LEVELS = 8;

// What the pilot and the task queue derive from the reach graph.
struct Topology {
    std::vector<int> level;                        // [S] longest path from a headwater
    std::vector<Launch> pilot;                     // the pilot's launches (those left with no reach are dropped)
    std::vector<int> down_ptr, down_idx, qslot;    // queue: downstream CSR; [S] ring buffer of a reach read downstream, or -1
    int n_route = 0, ring_chunks = 0;              // ring buffers, time chunks a ring buffer holds
};

Topology derive_topology(int S, const int32_t* up_ptr, const int32_t* up_idx, const Schedule& sch, int n_chunks)
{
    Topology t;
    t.level.assign(S, 0);
    for (int s = 0; s < S; ++s)
        for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) t.level[s] = std::max(t.level[s], t.level[up_idx[k]] + 1);
    for (const Launch& L : sch.launches) {
        Launch P;
        P.chain_ptr.push_back(0);
        for (size_t c = 0; c + 1 < L.chain_ptr.size(); ++c) {
            for (int i = L.chain_ptr[c]; i < L.chain_ptr[c + 1] && t.level[L.chain_reach[i]] < PILOT_LEVELS; ++i)
                P.chain_reach.push_back(L.chain_reach[i]);
            if ((int)P.chain_reach.size() > P.chain_ptr.back()) P.chain_ptr.push_back((int)P.chain_reach.size());
        }
        if (!P.chain_reach.empty()) t.pilot.push_back(std::move(P));
    }
    std::vector<int> n_down(S, 0);
    int max_jump = 0;
    for (int s = 0; s < S; ++s)
        for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) { max_jump = std::max(max_jump, t.level[s] - t.level[up_idx[k]]); ++n_down[up_idx[k]]; }
    t.ring_chunks = std::min(n_chunks, max_jump + 1);
    t.down_ptr.assign(S + 1, 0);
    t.down_idx.assign((size_t)std::max(1, (int)up_ptr[S]), 0);
    t.qslot.assign(S, -1);
    for (int s = 0; s < S; ++s) t.down_ptr[s + 1] = t.down_ptr[s] + n_down[s];
    { std::vector<int> fill(t.down_ptr.begin(), t.down_ptr.end() - 1);
      for (int s = 0; s < S; ++s) for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) t.down_idx[fill[up_idx[k]]++] = s; }
    for (int s = 0; s < S; ++s) if (n_down[s] > 0) t.qslot[s] = t.n_route++;
    return t;
}

template <int V> using Int = std::integral_constant<int, V>;

// Calls fn(integrator, snow, team, stiff), each a std::integral_constant, for the run's kernel: RK4, Cash-Karp and the fp32
// mirror at one lane per member, integrator 2 at one or four lanes with or without the stiff pair; each with snow on and off.
template <class F>
void dispatch_kernel(const simplyp_opts& opts, const RunShape& shape, F&& fn)
{
    auto with_snow = [&](auto integ, auto team, auto stiff) {
        if (opts.snow) fn(integ, std::true_type{}, team, stiff);
        else fn(integ, std::false_type{}, team, stiff);
    };
    auto with_team = [&](auto stiff) {          // integrator 2
        if (shape.team == 4) with_snow(Int<SIMPLYP_INTEG_CASHKARP_AUG>{}, Int<4>{}, stiff);
        else with_snow(Int<SIMPLYP_INTEG_CASHKARP_AUG>{}, Int<1>{}, stiff);
    };
    if (opts.integrator == SIMPLYP_INTEG_RK4) with_snow(Int<SIMPLYP_INTEG_RK4>{}, Int<1>{}, std::false_type{});
    else if (opts.integrator == SIMPLYP_INTEG_CASHKARP) with_snow(Int<SIMPLYP_INTEG_CASHKARP>{}, Int<1>{}, std::false_type{});
    else if (opts.integrator == SIMPLYP_INTEG_CASHKARP_AUG_F32) with_snow(Int<SIMPLYP_INTEG_CASHKARP_AUG_F32>{}, Int<1>{}, std::false_type{});
    else if (shape.stiff) with_team(std::true_type{});
    else with_team(std::false_type{});
}

// One launch of the chain kernel: n_chains mutually independent chains, at these offsets of the uploaded schedule block.
struct ChainLaunch { size_t off_ptr, off_reach; unsigned n_chains; };

int launch_chains(simplyp_ctx* ctx, const simplyp_opts& opts, const RunShape& shape, simplyp::KernelArgs k, const ChainLaunch& c,
                  unsigned n_windows = 1u)
{
    k.chain_ptr = (const int*)ctx->sched.ptr + c.off_ptr;
    k.chain_reach = (const int*)ctx->sched.ptr + c.off_reach;
    const dim3 grid(shape.gx, c.n_chains, n_windows), block(simplyp::WAVE, 1, 1);
    dispatch_kernel(opts, shape, [&](auto integ, auto snow, auto team, auto stiff) {
        hipLaunchKernelGGL((simplyp::simplyp_chain_kernel<integ, snow, team, stiff>), grid, block, 0, ctx->stream, k);
    });
    HIP_TRY(ctx, hipGetLastError());
    return SIMPLYP_OK;
}

// Uploads the int32 schedule block -- up_ptr | up_idx | route_slot | out_slot | per launch: chain_ptr | chain_reach, the
// schedule's launches, then the pilot's -- and zeroes the counters and the per-member outputs; `a` then points at both.
int upload_schedule(simplyp_ctx* ctx, const Schedule& sch, const Topology& topo, const int32_t* up_ptr, const int32_t* up_idx,
                    const int32_t* out_reaches, simplyp::KernelArgs& a, std::vector<ChainLaunch>& launches,
                    std::vector<ChainLaunch>& pilot)
{
    const int S = a.S;
    if (int rc = ensure(ctx, ctx->counters, simplyp_ctx::N_COUNTERS * sizeof(unsigned long long))) return rc;
    std::vector<int> out_slot(S, -1);
    if (out_reaches) for (int k = 0; k < a.n_out_reaches; ++k) out_slot[out_reaches[k]] = k;
    else std::iota(out_slot.begin(), out_slot.end(), 0);
    std::vector<int> host;
    auto put = [&](const int* v, size_t n) { const size_t at = host.size(); host.insert(host.end(), v, v + n); return at; };
    const size_t off_up_ptr = put(up_ptr, S + 1), off_up_idx = put(up_idx, up_ptr[S]);
    const size_t off_rslot = put(sch.route_slot.data(), S), off_oslot = put(out_slot.data(), S);
    auto put_launches = [&](const std::vector<Launch>& ls, std::vector<ChainLaunch>& to) {
        for (const Launch& L : ls) {
            const size_t off_ptr = put(L.chain_ptr.data(), L.chain_ptr.size());
            to.push_back({off_ptr, put(L.chain_reach.data(), L.chain_reach.size()), (unsigned)L.chain_ptr.size() - 1u});
        }
    };
    put_launches(sch.launches, launches);
    put_launches(topo.pilot, pilot);
    if (int rc = ensure(ctx, ctx->sched, host.size() * sizeof(int))) return rc;
    // pageable source: the copy is staged before hipMemcpyAsync returns, `host` may go out of scope
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sched.ptr, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.ptr, 0, simplyp_ctx::N_COUNTERS * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.status, 0, (size_t)a.E * sizeof(int32_t), ctx->stream));
    if (a.member_rhs) HIP_TRY(ctx, hipMemsetAsync(a.member_rhs, 0, (size_t)a.E * sizeof(uint32_t), ctx->stream));
    const int* dsched = (const int*)ctx->sched.ptr;
    a.up_ptr = dsched + off_up_ptr; a.up_idx = dsched + off_up_idx;
    a.route_slot = dsched + off_rslot; a.out_slot = dsched + off_oslot;
    a.counters = (unsigned long long*)ctx->counters.ptr;
    return SIMPLYP_OK;
}

// The pilot: PILOT_WINDOWS short runs from the initial conditions, each over a different stretch of the forcing (spread over
// the first two years when the run is long enough, so that the seasons are sampled), one cost counter per member and window.
// Then the members' lane-slot order (order_members), and slot-ordered copies of the parameter tables for `a`.
int balance_members(simplyp_ctx* ctx, const simplyp_opts& opts, const RunShape& shape, const Schedule& sch,
                    const std::vector<ChainLaunch>& pilot, simplyp::KernelArgs& a)
{
    const int E = a.E, S = a.S, D = a.D;
    constexpr int PILOT_WINDOWS = 8;
    const int win_days = std::max(1, shape.pilot_days / PILOT_WINDOWS);
    const int win_stride = std::max(win_days, std::min(80, (D - win_days) / (PILOT_WINDOWS - 1)));      // ~1.6 years covered
    static_assert(PILOT_WINDOWS == simplyp::ORD_WIN, "the device's ordering kernels are written for the pilot's windows");
    const bool on_device = order_on_device(E);
    const size_t order_in_out = (size_t)E * (PILOT_WINDOWS * sizeof(uint32_t) + sizeof(int32_t));
    if (int rc = ensure(ctx, ctx->balance, order_in_out + (on_device ? order_workspace_bytes(E) : 0))) return rc;
    uint32_t* d_cost = (uint32_t*)ctx->balance.ptr;
    int32_t* d_perm = (int32_t*)(d_cost + (size_t)PILOT_WINDOWS * E);
    HIP_TRY(ctx, hipMemsetAsync(d_cost, 0, (size_t)PILOT_WINDOWS * E * sizeof(uint32_t), ctx->stream));
    simplyp::KernelArgs p = a;
    p.D = win_days;                   // forcing rows keep their stride of D days
    p.route_days = win_days;
    const size_t win_route = (size_t)sch.n_slots * 4 * win_days * E;      // doubles of routing scratch per window
    if (sch.n_slots > 0) {
        if (int rc = ensure(ctx, ctx->route, (size_t)PILOT_WINDOWS * win_route * sizeof(double))) return rc;
        p.route = (double*)ctx->route.ptr;
    }
    // all windows in one launch per schedule level (blockIdx.z = window): 8 x 1563 waves fill the chip's rounds, where
    // 8 launches of 1563 waves would each leave a half-empty second round
    p.win_stride = win_stride;
    p.win_route_stride = (long long)win_route;
    p.member_rhs = d_cost;
    for (const ChainLaunch& c : pilot)
        if (int rc = launch_chains(ctx, opts, shape, p, c, (unsigned)PILOT_WINDOWS)) return rc;
    if (on_device) {
        if (int rc = order_members_device(ctx, d_cost, d_perm, (unsigned char*)ctx->balance.ptr + order_in_out, E)) return rc;
    } else {
        // SIMPLYP_DEBUG: the host's share of the pilot, step by step
        const bool dbg = getenv("SIMPLYP_DEBUG") != nullptr;
        using clk = std::chrono::steady_clock;
        auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
        if (dbg) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        clk::time_point t0 = clk::now();
        std::vector<uint32_t> cost((size_t)PILOT_WINDOWS * E);
        HIP_TRY(ctx, hipMemcpyAsync(cost.data(), d_cost, cost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const double ms_d2h = ms_since(t0);
        t0 = clk::now();
        std::vector<int32_t> perm;
        order_members(cost, PILOT_WINDOWS, E, perm);
        const double ms_order = ms_since(t0);
        t0 = clk::now();
        HIP_TRY(ctx, hipMemcpyAsync(d_perm, perm.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (dbg)
            fprintf(stderr, "[simplyp] member order on the host, E=%d: costs to the host %.3f ms, order_members %.3f ms, order to the device %.3f ms\n",
                    E, ms_d2h, ms_order, ms_since(t0));
    }
    // the pilot's bookkeeping must not leak into the real run
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.ptr, 0, simplyp_ctx::N_COUNTERS * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.status, 0, (size_t)E * sizeof(int32_t), ctx->stream));
    a.perm = d_perm;
    // slot-ordered copies of the parameter tables: the main kernels then read them coalesced
    const size_t n_mp = (size_t)SIMPLYP_NP_M * E, n_rp = (size_t)SIMPLYP_NP_R * S * E;
    const size_t bytes = (n_mp + n_rp) * sizeof(double) + (a.forcing_of_member ? (size_t)E * sizeof(int32_t) : 0);
    if (int rc = ensure(ctx, ctx->sorted_params, bytes)) return rc;
    double* s_mp = (double*)ctx->sorted_params.ptr;
    double* s_rp = s_mp + n_mp;
    int32_t* s_fom = (int32_t*)(s_rp + n_rp);
    const dim3 gb(256), gg((unsigned)((E + 255) / 256), 16);
    hipLaunchKernelGGL(simplyp::gather_columns_kernel<double>, gg, gb, 0, ctx->stream, a.mp, s_mp, d_perm, (int)SIMPLYP_NP_M, E);
    hipLaunchKernelGGL(simplyp::gather_columns_kernel<double>, gg, gb, 0, ctx->stream, a.rp, s_rp, d_perm, (int)SIMPLYP_NP_R * S, E);
    if (a.forcing_of_member)
        hipLaunchKernelGGL(simplyp::gather_columns_kernel<int32_t>, dim3(gg.x, 1), gb, 0, ctx->stream, a.forcing_of_member, s_fom, d_perm, 1, E);
    HIP_TRY(ctx, hipGetLastError());
    a.mp = s_mp; a.rp = s_rp;
    if (a.forcing_of_member) a.forcing_of_member = s_fom;
    a.params_by_slot = 1;
    return SIMPLYP_OK;
}

// Packed output stream: may this run's streamed table travel as packed records (simplyp_pack.h)?  The pack epilogue of the
// queue kernel handles the plain case only: daily rows of one reach, one lane per member, full waves, and lane slots that are
// contiguous in the table (columns in slot order, or no permutation at all).
bool pack_eligible(const simplyp_opts& opts, const RunShape& shape, const simplyp::KernelArgs& a)
{
    return shape.stream_chunks && opts.n_periods == 0 && a.S == 1 && a.n_out_reaches == 1 && shape.team == 1 &&
           shape.lanes == simplyp::WAVE && (a.out_by_slot || !a.perm);
}

// SIMPLYP_STREAM_PACK unset: pack only when the raw copies would clearly outlast the kernel.  Per day of
// the run, the raw table needs n_cols x E x 8 bytes at PACK_LINK_GBS on the link; the PACKING kernel needs
// PACK_KERNEL_NS_PER_MEMBER_DAY per member (the flagship with the row-adaptive epilogue: 579 ms for 100 000 members x 10 957
// days, profiles/r07_pack; 533.6 ms without any epilogue) but never less than one round of waves (PACK_KERNEL_US_PER_DAY_MIN:
// 480 ms measured for the 50 000-member shard that fills 782 of the 1024 wave slots, scaled by the same 579 / 533.6 -- that
// product is derived, not measured).  The packed rows cost 6.13 of 8 bytes per value on the model's table, so the packed copy
// takes 0.77 of the raw one: a run whose raw copy is 10 % longer than its packing kernel ends with the kernel (0.85 < 1) and
// gains those 10 %; one whose raw copy is no longer than the packing kernel gains nothing.
constexpr double PACK_LINK_GBS = 56.7, PACK_KERNEL_NS_PER_MEMBER_DAY = 0.528, PACK_KERNEL_US_PER_DAY_MIN = 47.5;
constexpr double PACK_COPY_OVER_KERNEL = 1.10;
constexpr bool PACK_AUTO_ON = true;       // the verdict of the full-size runs (profiles/r07_pack/README.md; r06_pack/gate.md before)

bool pack_wanted(const simplyp_opts& opts, const RunShape& shape, const simplyp::KernelArgs& a)
{
    if (!pack_eligible(opts, shape, a)) return false;
    if (const char* env = getenv("SIMPLYP_STREAM_PACK")) {
        if (env[0] == '0') return false;
        if (env[0] == '1') return true;
    }
    const double copy_us = (double)popcount32(a.out_mask) * a.E * 8.0 / (PACK_LINK_GBS * 1e3);
    const double kernel_us = std::max(PACK_KERNEL_US_PER_DAY_MIN, PACK_KERNEL_NS_PER_MEMBER_DAY * 1e-3 * a.E);
    return PACK_AUTO_ON && copy_us > PACK_COPY_OVER_KERNEL * kernel_us;
}

// Buffers of a packed table: the device records, sized for their capacity; their two counters each on the device and in pinned
// host memory (zeroed); behind the device counters the table's predictor columns (uploaded).  All of it is enqueued on
// ctx->stream.  `args` is what a packing kernel takes; its `buf` stays null when the records do not fit the device's free memory.
int ensure_pack_buffers(simplyp_ctx* ctx, const simplyp_pack::Table& t, simplyp_pack::PackArgs& args)
{
    const size_t n_records = (size_t)t.n_chunks() * (size_t)t.n_cols, n_words = 2 * n_records, bytes = n_records * t.stride;
    args = simplyp_pack::PackArgs{};
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (bytes > ctx->packed.bytes && bytes - ctx->packed.bytes > free_b / 10 * 9) return SIMPLYP_OK;
    if (int rc = ensure(ctx, ctx->packed, bytes)) return rc;
    if (int rc = ensure(ctx, ctx->pack_count, (n_words + (size_t)t.n_cols) * sizeof(unsigned))) return rc;
    if (n_words > ctx->host_pack_count_cap) {
        if (ctx->host_pack_count) { (void)hipHostFree(ctx->host_pack_count); ctx->host_pack_count = nullptr; ctx->host_pack_count_cap = 0; }
        HIP_TRY(ctx, hipHostMalloc((void**)&ctx->host_pack_count, n_words * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));
        ctx->host_pack_count_cap = n_words;
    }
    memset(ctx->host_pack_count, 0, n_words * sizeof(uint32_t));
    unsigned* count = (unsigned*)ctx->pack_count.ptr;
    HIP_TRY(ctx, hipMemsetAsync(count, 0, n_words * sizeof(unsigned), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(count + n_words, t.pred, (size_t)t.n_cols * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    args.buf = (unsigned char*)ctx->packed.ptr; args.count = count; args.host_count = ctx->host_pack_count;
    args.stride = t.stride; args.cap = t.cap; args.cols = t.n_cols; args.pred = (const int*)(count + n_words);
    return SIMPLYP_OK;
}

// Task-queue kernel: (reach, time chunk, member group) tasks pulled by one persistent wave per SIMD.  `queued` stays false, and
// nothing is enqueued, when the ring buffers of the routing series do not fit: the run then takes the chain kernel.
int launch_queue(simplyp_ctx* ctx, const simplyp_opts& opts, const RunShape& shape, const Topology& topo,
                 const simplyp::KernelArgs& a, bool& queued)
{
    const int E = a.E, S = a.S, G = (int)shape.gx, n_chunks = shape.n_chunks, chunk_days = shape.chunk_days;
    const size_t ring_days = (size_t)topo.ring_chunks * chunk_days;
    const size_t route_bytes = (size_t)topo.n_route * 4 * ring_days * E * sizeof(double);
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (route_bytes > ctx->route.bytes && route_bytes - ctx->route.bytes > free_b / 10 * 9) return SIMPLYP_OK;   // does not fit: chain kernel
    // (reach, chunk) pairs in dependency order: by level + chunk, then reach
    std::vector<int> pair_idx((size_t)S * n_chunks);
    std::iota(pair_idx.begin(), pair_idx.end(), 0);
    std::stable_sort(pair_idx.begin(), pair_idx.end(), [&](int x, int y) {
        const int kx = topo.level[x / n_chunks] + x % n_chunks, ky = topo.level[y / n_chunks] + y % n_chunks;
        return kx != ky ? kx < ky : x < y;
    });
    std::vector<int> qi;                       // task_reach | task_chunk | down_ptr | down_idx | qslot
    for (int v : pair_idx) qi.push_back(v / n_chunks);
    for (int v : pair_idx) qi.push_back(v % n_chunks);
    const size_t off_dptr = qi.size(); qi.insert(qi.end(), topo.down_ptr.begin(), topo.down_ptr.end());
    const size_t off_didx = qi.size(); qi.insert(qi.end(), topo.down_idx.begin(), topo.down_idx.end());
    const size_t off_qslot = qi.size(); qi.insert(qi.end(), topo.qslot.begin(), topo.qslot.end());
    const size_t flags_bytes = (((size_t)S * G + 4) * sizeof(unsigned) + 255) / 256 * 256;      // ticket, error, progress, (pad), done[S][G]
    const size_t ints_bytes = (qi.size() * sizeof(int) + 255) / 256 * 256;
    if (int rc = ensure(ctx, ctx->queue, flags_bytes + ints_bytes + (size_t)S * simplyp::CKPT_N * E * sizeof(double))) return rc;
    if (route_bytes) { if (int rc = ensure(ctx, ctx->route, route_bytes)) return rc; }
    simplyp::QueueArgs q;                      // (q.pack: off)
    q.chunk_count = nullptr; q.host_ready = nullptr;
    if (shape.stream_chunks) {
        if (int rc = ensure(ctx, ctx->chunk_count, (size_t)n_chunks * sizeof(unsigned))) return rc;
        if ((size_t)n_chunks > ctx->host_ready_cap) {
            if (ctx->host_ready) { (void)hipHostFree(ctx->host_ready); ctx->host_ready = nullptr; ctx->host_ready_cap = 0; }
            // COHERENT (fine-grained) host memory, asked for explicitly: a flag raised by a running kernel must reach the
            // polling host thread before the kernel ends, which only fine-grained memory promises
            HIP_TRY(ctx, hipHostMalloc((void**)&ctx->host_ready, (size_t)n_chunks * sizeof(uint32_t),
                                       hipHostMallocCoherent | hipHostMallocMapped));
            ctx->host_ready_cap = (size_t)n_chunks;
        }
        memset(ctx->host_ready, 0, (size_t)n_chunks * sizeof(uint32_t));
        HIP_TRY(ctx, hipMemsetAsync(ctx->chunk_count.ptr, 0, (size_t)n_chunks * sizeof(unsigned), ctx->stream));
        q.chunk_count = (unsigned*)ctx->chunk_count.ptr;
        q.host_ready = ctx->host_ready;
        // PP is almost a constant multiple of Msus: predicted from it when both are in the table.
        // Columns are in ascending SIMPLYP_OUT_* order, so a column's place is the number of mask bits below its own.
        int32_t pred[32];
        for (int32_t& k : pred) k = -1;
        const uint32_t bx = 1u << SIMPLYP_OUT_MSUS_FLUX, by = 1u << SIMPLYP_OUT_PP_FLUX;
        if ((a.out_mask & bx) && (a.out_mask & by)) pred[popcount32(a.out_mask & (by - 1u))] = popcount32(a.out_mask & (bx - 1u));
        simplyp_ctx::CopyPlan& cp = ctx->copy_plan;
        cp.table = simplyp_pack::make_table(popcount32(a.out_mask), a.D, a.n_out_reaches * E, chunk_days, pred);
        if (pack_wanted(opts, shape, a)) {
            if (int rc = ensure_pack_buffers(ctx, cp.table, q.pack)) return rc;
            cp.pack_dev = q.pack.buf;
        }
    }
    char* base = (char*)ctx->queue.ptr;
    HIP_TRY(ctx, hipMemsetAsync(base, 0, flags_bytes, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(base + flags_bytes, qi.data(), qi.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned* flags = (unsigned*)base;
    const int* dq = (const int*)(base + flags_bytes);
    q.ticket = flags; q.error = flags + 1; q.progress = flags + 2; q.done = flags + 4;
    q.task_reach = dq; q.task_chunk = dq + pair_idx.size();
    q.down_ptr = dq + off_dptr; q.down_idx = dq + off_didx;
    q.ckpt = (double*)(base + flags_bytes + ints_bytes);
    q.n_groups = G; q.n_pairs = (int)pair_idx.size(); q.chunk_days = chunk_days; q.ring_chunks = topo.ring_chunks;
    q.tasks_per_chunk = (unsigned)S * (unsigned)G;
    q.max_polls = 20000000u;      // x (s_sleep 64 ~ 2 us): ~40 s in which NO task of the run completed means something is broken
    if (const char* mp_env = getenv("SIMPLYP_QUEUE_MAX_POLLS")) q.max_polls = (unsigned)strtoul(mp_env, nullptr, 10);
    simplyp::KernelArgs k = a;
    k.route = (double*)ctx->route.ptr;
    k.route_days = (int)ring_days;
    k.route_slot = dq + off_qslot;
    const unsigned workers = (unsigned)std::min<long long>((long long)pair_idx.size() * G, ctx->n_simd_slots);
    HIP_TRY(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
    dispatch_kernel(opts, shape, [&](auto integ, auto snow, auto team, auto stiff) {
        if constexpr (integ != SIMPLYP_INTEG_RK4)      // (plan_run never queues RK4)
            hipLaunchKernelGGL((simplyp::simplyp_queue_kernel<integ, snow, team, stiff>), dim3(workers), dim3(simplyp::WAVE), 0,
                               ctx->stream, k, q);
    });
    HIP_TRY(ctx, hipGetLastError());
    if (getenv("SIMPLYP_DEBUG")) fprintf(stderr, "[simplyp] queue kernel launched: S=%d G=%d pairs=%zu chunk=%d ring=%d workers=%u max_polls=%u\n", S, G, pair_idx.size(), chunk_days, topo.ring_chunks, workers, q.max_polls);
    queued = true;
    return SIMPLYP_OK;
}

// The copy of the output table to the buffer simplyp_stream_out armed: chunk by chunk beside the queue kernel (`chunked`), or
// the whole table behind the last launch.
int arm_copy(simplyp_ctx* ctx, double* host_out, const simplyp_opts& opts, const simplyp::KernelArgs& a, bool chunked)
{
    simplyp_ctx::CopyPlan& cp = ctx->copy_plan;
    cp.dev = a.out; cp.host = host_out; cp.chunked = chunked;
    if (chunked) {
        if (cp.pack_dev) {
            // ring, dispatcher and decode pool first (the ring is allocated, and so first touched, by the calling thread)
            hipError_t err = ctx->pack.start(ctx->device, (size_t)cp.table.E, cp.table.stride, cp.table.n_chunks() * cp.table.n_cols,
                                             simplyp_pack::decode_threads());
            if (err != hipSuccess) {
                ctx->pack.finish();
                return fail(ctx, SIMPLYP_ERR_NOMEM, "packed output stream: the pinned staging ring failed: %s", hipGetErrorString(err));
            }
        }
        ctx->run_over.store(0, std::memory_order_release);
        ctx->copier = std::thread(copier_main, ctx);       // chunk by chunk, beside the kernel
    } else {
        // no time chunks in this run (chain kernel, RK4, time-reduced rows): the whole table follows the last launch
        const size_t rows = (size_t)(opts.n_periods > 0 ? opts.n_periods : a.D);
        HIP_TRY(ctx, hipMemcpyAsync(host_out, a.out, (size_t)popcount32(a.out_mask) * rows * (size_t)a.n_out_reaches * (size_t)a.E * sizeof(double),
                                    hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_copy_done, ctx->stream));
    }
    ctx->copy_pending = true;
    return SIMPLYP_OK;
}

// Tells the copier thread that the run is over (whatever chunk flag is still down stays down) and joins it: every chunk's
// copy is enqueued when it returns.
void stop_copier(simplyp_ctx* ctx)
{
    ctx->run_over.store(1, std::memory_order_release);
    if (ctx->copier.joinable()) ctx->copier.join();
    ctx->pack.finish();         // every landed record decoded, every ring slot released, the pool joined (no-op when not packed)
}

}  // namespace

extern "C" {

int simplyp_abi_version(void) { return SIMPLYP_ABI_VERSION; }

int simplyp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int simplyp_ctx_create(int device, simplyp_ctx** out)
{
    if (!out) return fail(nullptr, SIMPLYP_ERR_ARG, "out is NULL");
    *out = nullptr;
    int n = simplyp_device_count();
    if (device < 0 || device >= n)
        return fail(nullptr, SIMPLYP_ERR_DEVICE, "device %d not available (%d HIP device(s) visible)", device, n);
    simplyp_ctx* ctx = new (std::nothrow) simplyp_ctx();
    if (!ctx) return fail(nullptr, SIMPLYP_ERR_NOMEM, "out of host memory");
    ctx->device = device;
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (err == hipSuccess) { ctx->own_stream = true; err = hipEventCreate(&ctx->ev_start); }
    if (err == hipSuccess) err = hipEventCreate(&ctx->ev_stop);
    if (err == hipSuccess) err = hipEventCreate(&ctx->ev_main);
    for (hipEvent_t& ev : ctx->ev_lap) if (err == hipSuccess) err = hipEventCreate(&ev);
    if (err == hipSuccess) err = hipEventCreate(&ctx->ev_copy_done);
    for (int i = 0; i < simplyp_ctx::N_COPY_STREAMS && err == hipSuccess; ++i) {
        err = hipStreamCreateWithFlags(&ctx->copy_streams[i], hipStreamNonBlocking);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&ctx->ev_copy_join[i], hipEventDisableTiming);
    }
    ctx->copy_stream = ctx->copy_streams[0];
    if (err == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            ctx->n_simd_slots = prop.multiProcessorCount * 4;

    }
    if (err != hipSuccess) {
        fail(nullptr, SIMPLYP_ERR_DEVICE, "context creation on device %d failed: %s", device, hipGetErrorString(err));
        simplyp_ctx_destroy(ctx);
        return SIMPLYP_ERR_DEVICE;
    }
    *out = ctx;
    return SIMPLYP_OK;
}

int simplyp_ctx_set_stream(simplyp_ctx* ctx, void* stream)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "a run is pending; call simplyp_sync first");
    (void)hipSetDevice(ctx->device);
    if (!stream) {
        // back to a private stream: the one the context already owns is kept (no create/destroy per call)
        if (ctx->own_stream && ctx->stream) return SIMPLYP_OK;
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
        return SIMPLYP_OK;
    }
    if (ctx->own_stream && ctx->stream) { (void)hipStreamDestroy(ctx->stream); ctx->stream = nullptr; ctx->own_stream = false; }
    ctx->stream = (hipStream_t)stream;
    return SIMPLYP_OK;
}

void simplyp_ctx_destroy(simplyp_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    stop_copier(ctx);
    for (int i = 0; i < simplyp_ctx::N_COPY_STREAMS; ++i) {
        if (ctx->copy_streams[i]) { (void)hipStreamSynchronize(ctx->copy_streams[i]); (void)hipStreamDestroy(ctx->copy_streams[i]); }
        if (ctx->ev_copy_join[i]) (void)hipEventDestroy(ctx->ev_copy_join[i]);
    }
    ctx->pack.release();
    if (ctx->ev_copy_done) (void)hipEventDestroy(ctx->ev_copy_done);
    if (ctx->host_ready) (void)hipHostFree(ctx->host_ready);
    if (ctx->host_pack_count) (void)hipHostFree(ctx->host_pack_count);
    if (ctx->packed.ptr) (void)hipFree(ctx->packed.ptr);
    if (ctx->pack_count.ptr) (void)hipFree(ctx->pack_count.ptr);
    if (ctx->chunk_count.ptr) (void)hipFree(ctx->chunk_count.ptr);
    if (ctx->route.ptr) (void)hipFree(ctx->route.ptr);
    if (ctx->sched.ptr) (void)hipFree(ctx->sched.ptr);
    if (ctx->counters.ptr) (void)hipFree(ctx->counters.ptr);
    if (ctx->balance.ptr) (void)hipFree(ctx->balance.ptr);
    if (ctx->sorted_params.ptr) (void)hipFree(ctx->sorted_params.ptr);
    if (ctx->forcing_ident.ptr) (void)hipFree(ctx->forcing_ident.ptr);
    if (ctx->queue.ptr) (void)hipFree(ctx->queue.ptr);
    if (ctx->gof_lists.ptr) (void)hipFree(ctx->gof_lists.ptr);
    if (ctx->gof_partial.ptr) (void)hipFree(ctx->gof_partial.ptr);
    if (ctx->quant.ptr) (void)hipFree(ctx->quant.ptr);
    if (ctx->wquant.ptr) (void)hipFree(ctx->wquant.ptr);
    if (ctx->score.ptr) (void)hipFree(ctx->score.ptr);
    if (ctx->pareto.ptr) (void)hipFree(ctx->pareto.ptr);
    if (ctx->tquant.ptr) (void)hipFree(ctx->tquant.ptr);
    if (ctx->pred.ptr) (void)hipFree(ctx->pred.ptr);
    if (ctx->mcmc.ptr) (void)hipFree(ctx->mcmc.ptr);
    if (ctx->nm.ptr) (void)hipFree(ctx->nm.ptr);
    if (ctx->nsga2.ptr) (void)hipFree(ctx->nsga2.ptr);
    if (ctx->nm_work.ptr) (void)hipFree(ctx->nm_work.ptr);
    if (ctx->sobol.ptr) (void)hipFree(ctx->sobol.ptr);
    if (ctx->pf.ptr) (void)hipFree(ctx->pf.ptr);
    if (ctx->order.ptr) (void)hipFree(ctx->order.ptr);
    if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
    if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
    if (ctx->ev_main) (void)hipEventDestroy(ctx->ev_main);
    for (hipEvent_t ev : ctx->ev_lap) if (ev) (void)hipEventDestroy(ev);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* simplyp_last_error(const simplyp_ctx* ctx)
{
    return ctx ? ctx->error.c_str() : g_create_error.c_str();
}

int64_t simplyp_out_bytes(const simplyp_dims* dims, const simplyp_opts* opts, int32_t n_out_reaches)
{
    if (!dims || !opts) return 0;
    const int64_t nor = n_out_reaches > 0 ? n_out_reaches : dims->S;
    const int64_t rows = opts->n_periods > 0 ? opts->n_periods : dims->D;
    return (int64_t)popcount32(opts->out_mask & (SIMPLYP_MASK_ALL | SIMPLYP_MASK_D_SNOW)) * rows * nor * dims->E * (int64_t)sizeof(double);
}

int simplyp_plan(int32_t S, const int32_t* up_ptr, const int32_t* up_idx, int32_t* n_launches, int32_t* n_slots,
                 int32_t* launch_of_reach, int32_t* chain_of_reach, int32_t* pos_in_chain, int32_t* route_slot)
{
    return guarded(nullptr, [&]() -> int {
        if (S <= 0 || !up_ptr || (up_ptr[S] > 0 && !up_idx)) return fail(nullptr, SIMPLYP_ERR_ARG, "bad plan arguments");
        simplyp_ctx tmp;
        Schedule sch;
        int rc = build_schedule(&tmp, S, up_ptr, up_idx, sch);
        if (rc != SIMPLYP_OK) { g_create_error = tmp.error; return rc; }
        if (n_launches) *n_launches = (int32_t)sch.launches.size();
        if (n_slots) *n_slots = sch.n_slots;
        for (size_t l = 0; l < sch.launches.size(); ++l) {
            const Launch& L = sch.launches[l];
            for (size_t c = 0; c + 1 < L.chain_ptr.size(); ++c)
                for (int i = L.chain_ptr[c]; i < L.chain_ptr[c + 1]; ++i) {
                    const int s = L.chain_reach[i];
                    if (launch_of_reach) launch_of_reach[s] = (int32_t)l;
                    if (chain_of_reach) chain_of_reach[s] = (int32_t)c;
                    if (pos_in_chain) pos_in_chain[s] = i - L.chain_ptr[c];
                }
        }
        if (route_slot) for (int s = 0; s < S; ++s) route_slot[s] = sch.route_slot[s];
        return SIMPLYP_OK;
    });
}

static int run_async_body(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                          const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                          const int32_t* forcing_of_member,
                          const double* member_params, const double* reach_params,
                          const int32_t* up_ptr, const int32_t* up_idx,
                          const int32_t* out_reaches, int32_t n_out_reaches,
                          double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "a run is already pending on this context; call simplyp_sync");
    // streamed output armed by simplyp_stream_out: one-shot, consumed by THIS call whatever becomes of it -- a run refused for
    // its arguments must not leave the arm behind for a later run to fire into a buffer the caller has dropped since
    double* const host_out = ctx->stream_host;
    const int64_t host_out_bytes = ctx->stream_host_bytes;
    ctx->stream_host = nullptr; ctx->stream_host_bytes = 0;
    // the model state armed by simplyp_set_state: one-shot in the same way
    const double* const state_in = ctx->state_in;
    double* const state_out = ctx->state_out;
    ctx->state_in = nullptr; ctx->state_out = nullptr;
    if (int rc = check_args(ctx, dims, opts, forcing, doy, period_of_day, member_params, reach_params, up_ptr, up_idx, out,
                            member_status, member_of_slot, out_reaches, n_out_reaches, host_out, host_out_bytes))
        return rc;
    ctx->t_begin = std::chrono::steady_clock::now();
    ctx->copy_pending = false; ctx->copy_error = 0; ctx->streamed_chunks = 0;
    ctx->copy_plan = simplyp_ctx::CopyPlan{}; ctx->tally = simplyp_pack::Tally{};
    const int E = dims->E, S = dims->S, D = dims->D;
    Schedule sch;
    int rc = build_schedule(ctx, S, up_ptr, up_idx, sch);
    if (rc != SIMPLYP_OK) return rc;
    const RunShape shape = plan_run(*dims, *opts, ctx->n_simd_slots, host_out != nullptr);
    const Topology topo = derive_topology(S, up_ptr, up_idx, sch, shape.n_chunks);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    simplyp::KernelArgs a{};          // (zeros: no pilot window, members in their own order, tables by member)
    a.E = E; a.S = S; a.D = D; a.n_sets = dims->n_forcing_sets;
    a.forcing = forcing; a.doy = doy; a.forcing_of_member = forcing_of_member;
    a.period_of_day = period_of_day; a.n_periods = opts->n_periods;
    a.mp = member_params; a.rp = reach_params;
    a.out = out; a.status = member_status; a.member_rhs = member_rhs_evals;
    a.route = (double*)ctx->route.ptr;
    a.n_out_reaches = out_reaches ? n_out_reaches : S;
    a.out_mask = opts->out_mask & (SIMPLYP_MASK_ALL | SIMPLYP_MASK_D_SNOW);
    a.integrator = opts->integrator; a.substeps = opts->substeps; a.max_steps = opts->max_steps;
    a.dynamic_epc0 = opts->dynamic_epc0; a.dynamic_erod = opts->dynamic_erod;
    a.run_mode_cal = opts->run_mode_cal; a.sc_qr0 = opts->sc_qr0; a.project_vr = opts->project_vr;
    a.rtol = opts->rtol; a.atol = opts->atol; a.step_len = opts->step_len;
    a.D_stride = D; a.route_days = D;
    a.lanes = shape.lanes; a.team_shift = shape.team == 4 ? 2 : 0;
    std::vector<ChainLaunch> launches, pilot;
    if ((rc = upload_schedule(ctx, sch, topo, up_ptr, up_idx, out_reaches, a, launches, pilot)) != SIMPLYP_OK) return rc;
    // forcing uncertainty: the members' own sets first; the pilot and the main launches then read them like any per-member forcing
    if (opts->forcing_error && (rc = generate_forcing(ctx, *opts, a)) != SIMPLYP_OK) return rc;

    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    if (shape.balance && (rc = balance_members(ctx, *opts, shape, sch, pilot, a)) != SIMPLYP_OK) return rc;
    if (member_of_slot) {
        if (shape.balance) {
            HIP_TRY(ctx, hipMemcpyAsync(member_of_slot, a.perm, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            std::vector<int32_t> ident((size_t)E);
            std::iota(ident.begin(), ident.end(), 0);
            HIP_TRY(ctx, hipMemcpyAsync(member_of_slot, ident.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    a.out_by_slot = opts->out_slot_order ? 1 : 0;
    // warm start: set behind the pilot, which ranks the members' costs from the cold initial conditions and stores no state
    a.state_in = state_in; a.state_out = state_out;
    if (opts->n_periods > 0)       // running sums start from zero
        HIP_TRY(ctx, hipMemsetAsync(out, 0, (size_t)simplyp_out_bytes(dims, opts, a.n_out_reaches), ctx->stream));

    bool queued = false;
    if (shape.want_queue && (rc = launch_queue(ctx, *opts, shape, topo, a, queued)) != SIMPLYP_OK) return rc;
    if (!queued) {
        // whole-run daily series of every reach that is read downstream
        if (sch.n_slots > 0 && (rc = ensure(ctx, ctx->route, (size_t)sch.n_slots * 4 * D * E * sizeof(double))) != SIMPLYP_OK) return rc;
        a.route = (double*)ctx->route.ptr;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
        for (const ChainLaunch& c : launches)
            if ((rc = launch_chains(ctx, *opts, shape, a, c)) != SIMPLYP_OK) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->last = simplyp_stats{};
    ctx->last.lanes_per_wave = shape.lanes; ctx->last.lanes_per_member = shape.team; ctx->last.stiff_pair = shape.stiff;
    ctx->last.balanced = shape.balance; ctx->last.queued = queued; ctx->last.n_launches = queued ? 1 : (int)launches.size();
    if (host_out && (rc = arm_copy(ctx, host_out, *opts, a, queued && shape.stream_chunks)) != SIMPLYP_OK) return rc;
    ctx->pending = true;
    return SIMPLYP_OK;
}

// Whatever way simplyp_sync (or a failed launch) leaves: the copier thread is told the run is over and joined, both copy streams
// are idle, nothing of the library still writes to the caller's host buffer, and the context can start another streamed run
// (std::thread::operator= on a joinable thread would call std::terminate).
static void quiesce_streaming(simplyp_ctx* ctx)
{
    stop_copier(ctx);
    for (int i = 0; i < simplyp_ctx::N_COPY_STREAMS; ++i)
        if (ctx->copy_streams[i]) (void)hipStreamSynchronize(ctx->copy_streams[i]);
    ctx->copy_pending = false;
}

// Errors met after work has been enqueued must not leave it in flight behind the caller's back.
static int run_async_impl(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                          const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                          const int32_t* forcing_of_member,
                          const double* member_params, const double* reach_params,
                          const int32_t* up_ptr, const int32_t* up_idx,
                          const int32_t* out_reaches, int32_t n_out_reaches,
                          double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals)
{
    const int rc = run_async_body(ctx, dims, opts, forcing, doy, period_of_day, forcing_of_member, member_params, reach_params,
                                  up_ptr, up_idx, out_reaches, n_out_reaches, out, member_status, member_of_slot, member_rhs_evals);
    if (rc != SIMPLYP_OK && ctx && !ctx->pending) {
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        quiesce_streaming(ctx);
    }
    return rc;
}

int simplyp_run_async(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                      const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                      const int32_t* forcing_of_member,
                      const double* member_params, const double* reach_params,
                      const int32_t* up_ptr, const int32_t* up_idx,
                      const int32_t* out_reaches, int32_t n_out_reaches,
                      double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals)
{
    return guarded(ctx, [&] { return run_async_impl(ctx, dims, opts, forcing, doy, period_of_day, forcing_of_member, member_params, reach_params,
                                      up_ptr, up_idx, out_reaches, n_out_reaches, out, member_status, member_of_slot,
                                      member_rhs_evals); });
}

static int sync_impl(simplyp_ctx* ctx, simplyp_stats* stats)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (getenv("SIMPLYP_DEBUG")) fprintf(stderr, "[simplyp] sync: waiting for the stop event\n");
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (getenv("SIMPLYP_DEBUG")) fprintf(stderr, "[simplyp] sync: stream idle\n");
    float ms_tail = 0.f;
    double stream_gbs = 0.0;
    const bool copied = ctx->copy_pending;
    if (copied) {
        stop_copier(ctx);                                      // the launches are done
        if (!ctx->copy_error && ctx->pack.error()) ctx->copy_error = ctx->pack.error();
        if (ctx->copy_error)
            return fail(ctx, SIMPLYP_ERR_DEVICE, "streamed output: a device-to-host copy failed: %s", hipGetErrorString((hipError_t)ctx->copy_error));
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_copy_done));
        HIP_TRY(ctx, hipEventElapsedTime(&ms_tail, ctx->ev_stop, ctx->ev_copy_done));
        if (ctx->copy_plan.chunked) {
            // chunked run: the rate the table travelled at
            float ms_run = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms_run, ctx->ev_main, ctx->ev_copy_done));
            const simplyp_pack::Table& t = ctx->copy_plan.table;
            const double bytes = (double)t.n_cols * (double)t.rows * (double)t.E * sizeof(double);
            stream_gbs = ms_run > 0.f ? bytes / (ms_run * 1e-3) / 1e9 : 0.0;
        }
    }
    unsigned long long c[simplyp_ctx::N_COUNTERS] = {};
    HIP_TRY(ctx, hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    if (ctx->last.queued) {
        unsigned err = 0;
        HIP_TRY(ctx, hipMemcpy(&err, (unsigned*)ctx->queue.ptr + 1, sizeof(err), hipMemcpyDeviceToHost));
        if (err)
            return fail(ctx, SIMPLYP_ERR_DEVICE, "task-queue kernel: a wave waited for a time chunk while no task of the run completed for "
                        "%llu polls (bound: SIMPLYP_QUEUE_MAX_POLLS); results are incomplete", c[6]);
    }
    if (copied && ctx->copy_plan.pack_dev && getenv("SIMPLYP_DEBUG"))
        fprintf(stderr, "[simplyp] packed stream: %d records packed (%zu bytes on the link), %d raw (%zu bytes on the link: %d past the "
                "capacity, %d not smaller than raw, %d follow a raw predictor column)\n", ctx->tally.n_packed, ctx->tally.link_bytes,
                ctx->tally.n_raw, ctx->tally.raw_bytes, ctx->tally.raw_why[simplyp_pack::RAW_PAST_CAPACITY],
                ctx->tally.raw_why[simplyp_pack::RAW_NOT_SMALLER], ctx->tally.raw_why[simplyp_pack::RAW_FOLLOWS]);
    if (copied && ctx->copy_plan.pack_dev && ctx->tally.n_raw && getenv("SIMPLYP_DEBUG"))
        for (int j = 0; j < ctx->copy_plan.table.n_cols; ++j) fprintf(stderr, "[simplyp] packed stream: column %d: %d raw\n", j, ctx->tally.raw_of_col[j]);
    if (stats) {
        float ms = 0.f, ms_pilot = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_main, ctx->ev_stop));
        HIP_TRY(ctx, hipEventElapsedTime(&ms_pilot, ctx->ev_start, ctx->ev_main));
        *stats = ctx->last;                                    // the fields the run's shape decided, the rest zero
        stats->rhs_evals = c[0]; stats->steps = c[1]; stats->rejected = c[2];
        stats->kernel_ms = ms;
        // lanes doing useful work per issued attempt: (attempts summed over lanes) / (64 x wave-level attempts)
        // (of all 64 lanes, also when a wave carries fewer members; a member spread over several lanes occupies them all)
        stats->simt_efficiency = c[3] ? (double)(c[0] / 6) * ctx->last.lanes_per_member / (64.0 * (double)c[3]) : 1.0;
        stats->pilot_ms = ctx->last.balanced ? ms_pilot : 0.0;
        stats->streamed_chunks = copied ? ctx->streamed_chunks : 0;
        stats->d2h_tail_ms = copied ? ms_tail : 0.0;
        stats->stream_gbs = stream_gbs;
        stats->queue_waits = ctx->last.queued ? c[4] : 0;
        stats->queue_longest_wait_polls = ctx->last.queued ? (uint32_t)c[5] : 0;
        if (copied && ctx->copy_plan.pack_dev) {
            stats->packed_records = (int32_t)(((uint32_t)ctx->tally.n_raw << 16) | ((uint32_t)ctx->tally.n_packed & 0xFFFFu));
            stats->pack_overflow_blocks = ctx->tally.n_overflow;
        }
        stats->queue_longest_stall_polls = ctx->last.queued ? c[6] : 0;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->t_begin).count();
    }
    return SIMPLYP_OK;
}

int simplyp_sync(simplyp_ctx* ctx, simplyp_stats* stats)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (!ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "no run pending");
    ctx->pending = false;
    int rc;
    try {
        rc = sync_impl(ctx, stats);
    } catch (const std::exception& e) {
        rc = fail(ctx, SIMPLYP_ERR_DEVICE, "unexpected host error: %s", e.what());
    }
    quiesce_streaming(ctx);      // on every exit, error or not (a second join / synchronize is a no-op)
    // The packed records are as large as the table they mirror (44 GB for C3): the buffer stays for the next packed run of the
    // same kind, but a context that has moved on to other work gives it back, outside the run's wall time
    if (!ctx->copy_plan.pack_dev && ctx->packed.ptr) { (void)hipFree(ctx->packed.ptr); ctx->packed.ptr = nullptr; ctx->packed.bytes = 0; }
    return rc;
}

int simplyp_stream_out(simplyp_ctx* ctx, double* host_out, int64_t host_bytes)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "a run is pending on this context; call simplyp_sync first");
    if (host_out && host_bytes <= 0) return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_stream_out: host_bytes must be > 0");
    ctx->stream_host = host_out;
    ctx->stream_host_bytes = host_out ? host_bytes : 0;
    return SIMPLYP_OK;
}

// simplyp_fetch_packed: the table is packed by one wave per (chunk, 64-double group), then every record takes the copier's and
// the decode pool's path of a packed run (raw records are copied from the table, as there).
// pred_col: simplyp_pack::pred_cols_ok.
static int fetch_packed_impl(simplyp_ctx* ctx, const double* dev_table, int32_t n_cols, int32_t rows, int32_t row_doubles,
                             int32_t chunk_days, const int32_t* pred_col, double* host_out, int64_t host_bytes, int32_t* counts,
                             int64_t* bytes)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "a run is pending on this context; call simplyp_sync first");
    if (!dev_table || !host_out || n_cols <= 0 || rows <= 0 || row_doubles <= 0 || chunk_days <= 0)
        return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_fetch_packed: bad table arguments");
    if (!simplyp_pack::pred_cols_ok(pred_col, n_cols))
        return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_fetch_packed: at most 32 columns, and pred_col[j] must be -1 or a column before j");
    const size_t table_bytes = (size_t)n_cols * rows * row_doubles * sizeof(double);
    if (host_bytes < (int64_t)table_bytes)
        return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_fetch_packed: host buffer of %lld bytes is smaller than the table (%zu)", (long long)host_bytes, table_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const simplyp_pack::Table t = simplyp_pack::make_table(n_cols, rows, row_doubles, (chunk_days + 63) / 64 * 64, pred_col);
    const int n_rec = t.n_chunks() * n_cols;
    if (t.n_chunks() > 65535) return fail(ctx, SIMPLYP_ERR_ARG, "simplyp_fetch_packed: more than 65535 chunks");
    simplyp_pack::PackArgs args;
    if (int rc = ensure_pack_buffers(ctx, t, args)) return rc;
    if (!args.buf) return fail(ctx, SIMPLYP_ERR_NOMEM, "simplyp_fetch_packed: the packed records do not fit the device's free memory");
    hipLaunchKernelGGL(simplyp::simplyp_pack_table_kernel, dim3((unsigned)((row_doubles + simplyp_pack::GROUP - 1) / simplyp_pack::GROUP), (unsigned)t.n_chunks()),
                       dim3(simplyp::WAVE), 0, ctx->stream, dev_table, rows, row_doubles, t.chunk_days, args);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->host_pack_count, args.count, 2 * (size_t)n_rec * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hipError_t err = ctx->pack.start(ctx->device, (size_t)row_doubles, t.stride, n_rec, simplyp_pack::decode_threads());
    simplyp_pack::Tally tally;
    unsigned n_issued = 0;
    // the copier's path: the same two streams in turn, and nothing more once a call has failed
    auto next_stream = [&] { return ctx->copy_streams[n_issued++ % (unsigned)simplyp_ctx::N_COPY_STREAMS]; };
    for (int c = 0; c < t.n_chunks(); ++c) {
        const uint32_t* count = ctx->host_pack_count + 2 * t.record(c, 0);
        simplyp_pack::route_chunk(
            t, c, args.buf, host_out, tally,
            [&](int j, unsigned& overflow_blocks, size_t& words) { overflow_blocks = count[2 * j]; words = count[2 * j + 1]; },
            [&](const simplyp_pack::PackJob& job) { if (err == hipSuccess) err = ctx->pack.submit(job, next_stream()); },
            [&](size_t off, size_t bytes) {
                if (err == hipSuccess) err = hipMemcpyAsync(host_out + off, dev_table + off, bytes, hipMemcpyDeviceToHost, next_stream());
            });
    }
    for (int i = 0; i < simplyp_ctx::N_COPY_STREAMS; ++i) {
        hipError_t e2 = hipStreamSynchronize(ctx->copy_streams[i]);
        if (err == hipSuccess) err = e2;
    }
    ctx->pack.finish();
    if (err == hipSuccess && ctx->pack.error()) err = (hipError_t)ctx->pack.error();
    if (err != hipSuccess) return fail(ctx, SIMPLYP_ERR_DEVICE, "simplyp_fetch_packed: %s", hipGetErrorString(err));
    if (counts) { counts[0] = tally.n_packed; counts[1] = (int32_t)tally.n_overflow; counts[2] = tally.n_raw; }
    if (bytes) { bytes[0] = (int64_t)tally.link_bytes; bytes[1] = (int64_t)tally.n_packed * row_doubles * (int64_t)sizeof(double); }
    return SIMPLYP_OK;
}

int simplyp_fetch_packed(simplyp_ctx* ctx, const double* dev_table, int32_t n_cols, int32_t rows, int32_t row_doubles,
                         int32_t chunk_days, double* host_out, int64_t host_bytes, int32_t* counts)
{
    return guarded(ctx, [&] { return fetch_packed_impl(ctx, dev_table, n_cols, rows, row_doubles, chunk_days, nullptr, host_out, host_bytes, counts, nullptr); });
}

int simplyp_fetch_packed_pred(simplyp_ctx* ctx, const double* dev_table, int32_t n_cols, int32_t rows, int32_t row_doubles,
                              int32_t chunk_days, const int32_t* pred_col, double* host_out, int64_t host_bytes, int32_t* counts,
                              int64_t* bytes)
{
    return guarded(ctx, [&] { return fetch_packed_impl(ctx, dev_table, n_cols, rows, row_doubles, chunk_days, pred_col, host_out, host_bytes, counts, bytes); });
}

static int pack_roundtrip_host_impl(const double* table, int32_t n_cols, int32_t rows, int32_t row_doubles, int32_t chunk_days,
                                    const int32_t* pred_col, double* out, int32_t* counts, int64_t* bytes)
{
    if (!table || !out || n_cols <= 0 || rows <= 0 || row_doubles <= 0 || chunk_days <= 0)
        return fail(nullptr, SIMPLYP_ERR_ARG, "simplyp_pack_roundtrip_host: bad table arguments");
    if (!simplyp_pack::pred_cols_ok(pred_col, n_cols))
        return fail(nullptr, SIMPLYP_ERR_ARG, "simplyp_pack_roundtrip_host: at most 32 columns, and pred_col[j] must be -1 or a column before j");
    const simplyp_pack::Table t = simplyp_pack::make_table(n_cols, rows, row_doubles, (chunk_days + 63) / 64 * 64, pred_col);
    const size_t E = (size_t)row_doubles, G = (E + simplyp_pack::GROUP - 1) / simplyp_pack::GROUP;
    std::vector<unsigned char> rec(t.stride);       // one record at a time: encoded when the router asks for its counters
    simplyp_pack::Tally tally;
    constexpr size_t RANGES = 3;    // the decoder works on member ranges of whole blocks, as the pool's threads do
    simplyp_pack::FpDefault fp;     // (the decode threads hold one each)
    (void)fp;
    for (int c = 0; c < t.n_chunks(); ++c)
        simplyp_pack::route_chunk(
            t, c, nullptr, out, tally,
            [&](int j, unsigned& overflow_blocks, size_t& words) {
                const int k = t.pred[j];
                uint64_t cnt[2];
                simplyp_pack::encode_record_host(table + t.offset(j, c), k >= 0 ? table + t.offset(k, c) : nullptr, E, t.days(c), E, rec.data(),
                                                 t.layout_of(c), cnt);
                overflow_blocks = (unsigned)cnt[0]; words = (size_t)cnt[1];
            },
            [&](const simplyp_pack::PackJob& job) {
                for (size_t r = 0; r < RANGES; ++r) {
                    const size_t e0 = G * r / RANGES * simplyp_pack::GROUP, e1 = std::min(E, G * (r + 1) / RANGES * simplyp_pack::GROUP);
                    if (e1 > e0) simplyp_pack::decode_range(rec.data(), job.L, job.nd, E, e0, e1, job.dst, job.xdst, job.stride);
                }
                __builtin_ia32_sfence();
            },
            [&](size_t off, size_t bytes) { memcpy(out + off, table + off, bytes); });
    if (counts) { counts[0] = tally.n_packed; counts[1] = (int32_t)tally.n_overflow; counts[2] = tally.n_raw; }
    if (bytes) { bytes[0] = (int64_t)tally.link_bytes; bytes[1] = (int64_t)tally.n_packed * (int64_t)E * (int64_t)sizeof(double); }
    return SIMPLYP_OK;
}

int simplyp_pack_roundtrip_host(const double* table, int32_t n_cols, int32_t rows, int32_t row_doubles, int32_t chunk_days,
                                double* out, int32_t* counts)
{
    return guarded(nullptr, [&] { return pack_roundtrip_host_impl(table, n_cols, rows, row_doubles, chunk_days, nullptr, out, counts, nullptr); });
}

int simplyp_pack_roundtrip_host_pred(const double* table, int32_t n_cols, int32_t rows, int32_t row_doubles, int32_t chunk_days,
                                     const int32_t* pred_col, double* out, int32_t* counts, int64_t* bytes)
{
    return guarded(nullptr, [&] { return pack_roundtrip_host_impl(table, n_cols, rows, row_doubles, chunk_days, pred_col, out, counts, bytes); });
}

int64_t simplyp_state_bytes(const simplyp_dims* dims)
{
    if (!dims || dims->E <= 0 || dims->S <= 0) return -1;
    return (int64_t)dims->S * SIMPLYP_N_STATE * (int64_t)dims->E * (int64_t)sizeof(double);
}

int simplyp_set_state(simplyp_ctx* ctx, const double* state_in, double* state_out)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    if (ctx->pending) return fail(ctx, SIMPLYP_ERR_ARG, "a run is pending on this context; call simplyp_sync first");
    ctx->state_in = state_in;
    ctx->state_out = state_out;
    return SIMPLYP_OK;
}

int simplyp_run(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                const int32_t* forcing_of_member,
                const double* member_params, const double* reach_params,
                const int32_t* up_ptr, const int32_t* up_idx,
                const int32_t* out_reaches, int32_t n_out_reaches,
                double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals,
                simplyp_stats* stats)
{
    int rc = simplyp_run_async(ctx, dims, opts, forcing, doy, period_of_day, forcing_of_member, member_params, reach_params,
                               up_ptr, up_idx, out_reaches, n_out_reaches, out, member_status, member_of_slot,
                               member_rhs_evals);
    if (rc != SIMPLYP_OK) return rc;
    return simplyp_sync(ctx, stats);
}

namespace st = simplyp_table;
static_assert(st::TARGET_F_TDP == simplyp::MCMC_TARGET_F_TDP && st::TARGET_NONE == simplyp::MCMC_TARGET_NONE, "one meaning of a target");

// A rule of simplyp_table.h that says no: its message (`msg`, which `call` names) becomes the context's.
#define TABLE_TRY(ctx, call)                                                    \
    do {                                                                        \
        std::string msg;                                                        \
        if (int rc__ = (call)) return fail(ctx, rc__, "%s", msg.c_str());       \
    } while (0)

// The frame of an analysis entry: constructed by entry() with the context and the entry's name, opened, and then the one
// place that says how an entry is refused, timed and checked.  open() states, in this order: a NULL context is SIMPLYP_ERR_ARG; a
// context with a run pending is refused (ev_start / ev_stop below are that run's until simplyp_sync has read them); the
// context's device becomes current.  Nothing of an entry runs before open() has passed.
struct Entry {
    simplyp_ctx* ctx;
    const char* me;

    int open() const
    {
        if (!ctx) return SIMPLYP_ERR_ARG;
        if (ctx->pending) return refuse("a run is pending on this context; call simplyp_sync first");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        return SIMPLYP_OK;
    }

    // SIMPLYP_ERR_ARG with the message "<me>: <text>".
    __attribute__((format(printf, 2, 3))) int refuse(const char* fmt, ...) const
    {
        char text[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return fail(ctx, SIMPLYP_ERR_ARG, "%s: %s", me, text);
    }

    // After a launch.
    int launched() const { HIP_TRY(ctx, hipGetLastError()); return SIMPLYP_OK; }

    // The timed bracket: ev_start before the entry's launches; after them the check of the last launch, ev_stop, the read-back
    // of the entry's device counters if it has any (`bytes` from `src` to `dst`), and the wait for all of it.  *ms (an info's
    // kernel_ms, or NULL): ev_start to ev_stop.
    int begin() const { HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream)); return SIMPLYP_OK; }

    int end(double* ms, void* dst = nullptr, const void* src = nullptr, size_t bytes = 0) const
    {
        if (int rc = launched()) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
        if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float f = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&f, ctx->ev_start, ctx->ev_stop));
        if (ms) *ms = f;
        return SIMPLYP_OK;
    }
};

// An analysis entry: its frame opened, then its body, under guarded().
extern "C++" {
template <class F>
static int entry(simplyp_ctx* ctx, const char* name, F&& body)
{
    return guarded(ctx, [&]() -> int {
        const Entry e{ctx, name};
        if (int rc = e.open()) return rc;
        return body(e);
    });
}
}  // extern "C++"

// Host lists bound for one device buffer: the int32 lists (padded to an even count), then the double lists, in one upload.
struct Staging {
    std::vector<int32_t> ints;
    std::vector<double> dbl;
    const int32_t* d_ints = nullptr;       // after upload(): where the lists are on the device
    const double* d_dbl = nullptr;

    size_t put(const std::vector<int32_t>& v) { const size_t at = ints.size(); ints.insert(ints.end(), v.begin(), v.end()); return at; }
    size_t put(const std::vector<double>& v) { const size_t at = dbl.size(); dbl.insert(dbl.end(), v.begin(), v.end()); return at; }
    size_t bytes()
    {
        if (ints.size() & 1) ints.push_back(0);
        return ints.size() * sizeof(int32_t) + dbl.size() * sizeof(double);
    }
    // To `base`, which has room for bytes(), on the entry's stream.  The lists must outlive the copies: pageable memory is staged
    // before the call returns, and every entry synchronises its stream before it returns in any case.
    int upload(const Entry& e, void* base)
    {
        simplyp_ctx* const ctx = e.ctx;
        const size_t ibytes = ints.size() * sizeof(int32_t), dbytes = dbl.size() * sizeof(double);
        d_ints = (const int32_t*)base;
        d_dbl = (const double*)((char*)base + ibytes);
        if (ibytes) HIP_TRY(ctx, hipMemcpyAsync(base, ints.data(), ibytes, hipMemcpyHostToDevice, ctx->stream));
        if (dbytes) HIP_TRY(ctx, hipMemcpyAsync((char*)base + ibytes, dbl.data(), dbytes, hipMemcpyHostToDevice, ctx->stream));
        return SIMPLYP_OK;
    }
};

static int fill_nan(const Entry& e, double* ptr, long long n)
{
    hipLaunchKernelGGL(simplyp::quantile_fill_nan_kernel, dim3(blocks(n, 256)), dim3(256), 0, e.ctx->stream, ptr, n);
    return e.launched();
}

// An entry's device counters, `bytes` at the head of `buf` (grown to `room`): zeroed on the entry's stream.
static int zeroed_head(const Entry& e, DeviceBuf& buf, size_t room, size_t bytes)
{
    simplyp_ctx* const ctx = e.ctx;
    if (int rc = ensure(ctx, buf, room)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(buf.ptr, 0, bytes, ctx->stream));
    return SIMPLYP_OK;
}

// The table simplyp_gof, simplyp_gof_spearman and simplyp_waterbody read: its sizes, its output reaches, and the slots among
// its columns of the four series the statistics and sums are built from.
struct TableView : st::View {
    int col[4];
};

// Checks shared by the table reductions (`ptrs_ok`: the caller's required pointers are set).  waterbody == true: `out` is a
// table written by simplyp_waterbody, `out_mask` its wb_mask, and the series its summed discharge and fluxes.
static int check_table(const Entry& e, const simplyp_dims* dims, uint32_t out_mask, const int32_t* out_reaches,
                       int32_t n_out_reaches, bool ptrs_ok, bool waterbody, TableView& t)
{
    if (!dims || dims->E <= 0 || (!waterbody && dims->S <= 0) || dims->D <= 0) return e.refuse("bad dims");
    if (!ptrs_ok) return e.refuse("a required pointer is NULL");
    simplyp_dims d = *dims;
    if (waterbody) d.S = 1;
    TABLE_TRY(e.ctx, st::view(e.me, d, out_mask, waterbody ? SIMPLYP_WB_MASK_ALL : st::DAILY_COLUMNS, out_reaches, n_out_reaches, t, msg));
    if (!st::flux_slots(out_mask, waterbody ? st::WB_FLUX_COLS : st::FLUX_COLS, t.col))
        return e.refuse(waterbody ? "wb_mask must contain Q_cumecs, Msus_kg/day, TDP_kg/day and PP_kg/day"
                                  : "out_mask must contain Qr, Msus_kg/day, TDP_kg/day and PP_kg/day");
    return SIMPLYP_OK;
}

// The observation side of simplyp_gof and simplyp_gof_lag, shared by all members: counts, conditioning shifts, and per output
// reach the compact lists of discharge days and of chemistry days, each entry with whether it is the day after the entry before it.
struct ObsLists {
    std::vector<double> n_obs, shift;              // [R][6], [R][12]
    std::vector<int32_t> q_ptr, c_ptr, q_day, c_day, q_succ, c_succ;
    std::vector<double> q_obs, c_obs;              // [Kq][4], [Kc][20]: GofArgs
};

static void obs_lists(const double* obs, int R, int D, ObsLists& L)
{
    constexpr int NV = SIMPLYP_N_GOF_VARS;
    L.n_obs.assign((size_t)R * NV, 0.0);
    L.shift.assign((size_t)R * 12, 0.0);
    L.q_ptr.assign(R + 1, 0);
    L.c_ptr.assign(R + 1, 0);
    std::vector<double>&n_obs = L.n_obs, &shift = L.shift, &q_obs = L.q_obs, &c_obs = L.c_obs;
    std::vector<int32_t>&q_ptr = L.q_ptr, &c_ptr = L.c_ptr, &q_day = L.q_day, &c_day = L.c_day;
    const double nan = std::nan("");
    // the first entry of a reach's list is nobody's successor: the list before it is another reach's
    auto push_day = [](std::vector<int32_t>& day, std::vector<int32_t>& succ, size_t first, int d) {
        succ.push_back(day.size() > first && day.back() == d - 1 ? 1 : 0);
        day.push_back(d);
    };
    for (int r = 0; r < R; ++r) {
        const double* ob = obs + (size_t)r * NV * D;
        bool use[NV];
        for (int v = 0; v < NV; ++v) {
            double n = 0.0, so = 0.0, slo = 0.0, nlo = 0.0;
            for (int d = 0; d < D; ++d) {
                const double o = ob[(size_t)v * D + d];
                if (o == o) {
                    n += 1.0; so += o;
                    const double l = std::log(o);
                    if (l == l) { slo += l; nlo += 1.0; }        // a negative observation has no log: skipped, as gof_add skips it
                }
            }
            use[v] = n > 10.0;                                   // visualise_results.py:430
            n_obs[(size_t)r * NV + v] = n;
            shift[(size_t)r * 12 + v] = use[v] ? so / n : 0.0;
            // the log shift is only a conditioning constant: keep it finite when an observation is 0
            const double ml = use[v] && nlo > 0.0 ? slo / nlo : 0.0;
            shift[(size_t)r * 12 + 6 + v] = std::isfinite(ml) ? ml : 0.0;
        }
        // per observation: the value, its log, the log less its shift and 1 -- or 0 and 0 when there is no log (obs < 0)
        auto put_obs = [&](double o, int v, double* at, int stride) {
            const double l = std::log(o);
            at[0] = o; at[stride] = l;
            at[2 * stride] = l == l ? l - shift[(size_t)r * 12 + 6 + v] : 0.0;
            at[3 * stride] = l == l ? 1.0 : 0.0;
        };
        for (int d = 0; d < D; ++d) {
            const double q = ob[d];
            if (use[0] && q == q) {
                double row[4];
                put_obs(q, 0, row, 1);
                push_day(q_day, L.q_succ, (size_t)q_ptr[r], d);
                q_obs.insert(q_obs.end(), row, row + 4);
            }
            bool any = false;
            double row[20];
            for (int v = 1; v < NV; ++v) {
                const double o = ob[(size_t)v * D + d];
                const bool have = use[v] && o == o;
                if (have) put_obs(o, v, row + v - 1, 5);
                else for (int j = 0; j < 4; ++j) row[v - 1 + 5 * j] = nan;
                any = any || have;
            }
            if (any) { push_day(c_day, L.c_succ, (size_t)c_ptr[r], d); c_obs.insert(c_obs.end(), row, row + 20); }
        }
        q_ptr[r + 1] = (int32_t)q_day.size();
        c_ptr[r + 1] = (int32_t)c_day.size();
    }
}

// What simplyp_gof and simplyp_gof_lag set up alike once the table has passed: the lists on the device, the slices per day list,
// the partial-sum workspace for `nacc` running sums per variable, and the kernels' common arguments.  `partial_q` / `partial_c`:
// the entry's own discharge and chemistry kernels, whose occupancy the slice rule reads.
struct GofSetup {
    ObsLists L;
    simplyp::GofArgs g{};
    const int32_t* d_q_succ = nullptr;
    const int32_t* d_c_succ = nullptr;
    int groups = 0;
};

static int gof_setup(const Entry& e, const TableView& t, const double* out, const int32_t* member_of_slot, const double* f_tdp,
                     const double* reach_params, const double* obs, bool waterbody, int nacc, const void* partial_q,
                     const void* partial_c, GofSetup& u)
{
    simplyp_ctx* const ctx = e.ctx;
    constexpr int NV = SIMPLYP_N_GOF_VARS;
    const int E = t.E, S = t.S, D = t.D, R = t.R;
    obs_lists(obs, R, D, u.L);
    ObsLists& L = u.L;
    simplyp::GofArgs& g = u.g;
    std::copy(t.col, t.col + 4, g.col);

    const int groups = u.groups = (int)blocks(E, simplyp::WAVE);
    // Slices per day list. All waves of a launch take the same time, so what matters is how many rounds the chip needs:
    // pick the slice count with the fewest (rounds / slices), the smallest one within 3 % of the best (every slice costs a
    // row of partial sums), and keep at least 32 days per slice.
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
    auto pick_chunks = [&](const void* kernel, size_t list_len) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, simplyp::WAVE, 0) != hipSuccess || per_cu < 1) per_cu = 4;
        const double cap = (double)per_cu * prop.multiProcessorCount;
        const long long waves1 = (long long)groups * R;
        const int n_max = (int)std::max<long long>(1, std::min<long long>(64, (long long)(list_len / (size_t)R) / 32));
        int best = 1;
        double best_cost = 1e300;
        for (int n = 1; n <= n_max; ++n) {
            const double cost = std::ceil((double)waves1 * n / cap) / n;
            if (cost < best_cost * 0.97) { best = n; best_cost = cost; }
        }
        return best;
    };
    const int n_chunks_q = pick_chunks(partial_q, L.q_day.size());
    const int n_chunks_c = pick_chunks(partial_c, L.c_day.size());
    const int n_chunks = std::max(n_chunks_q, n_chunks_c);

    // one upload: int32 block then double block
    Staging up;
    const size_t o_reach = up.put(t.reach_of), o_qp = up.put(L.q_ptr), o_cp = up.put(L.c_ptr), o_qd = up.put(L.q_day), o_cd = up.put(L.c_day);
    const size_t o_qs = up.put(L.q_succ), o_cs = up.put(L.c_succ);
    const size_t o_qo = up.put(L.q_obs), o_co = up.put(L.c_obs), o_sh = up.put(L.shift), o_n = up.put(L.n_obs);
    if (int rc = ensure(ctx, ctx->gof_lists, up.bytes())) return rc;
    const size_t pbytes = (size_t)n_chunks * R * (NV * nacc) * E * sizeof(double);
    if (int rc = ensure(ctx, ctx->gof_partial, pbytes)) return rc;
    if (int rc = up.upload(e, ctx->gof_lists.ptr)) return rc;
    const int32_t* di = up.d_ints;
    const double* dd = up.d_dbl;
    g.E = E; g.R = R; g.D = D;
    g.out = out;
    g.col_stride = (long long)D * R * E;
    g.member_of_slot = member_of_slot;
    g.f_tdp = f_tdp;
    g.a_catch = waterbody ? nullptr : reach_params + (size_t)SIMPLYP_PR_A_CATCH * S * E;
    g.reach_of = di + o_reach; g.q_ptr = di + o_qp; g.c_ptr = di + o_cp; g.q_day = di + o_qd; g.c_day = di + o_cd;
    u.d_q_succ = di + o_qs; u.d_c_succ = di + o_cs;
    g.q_obs = dd + o_qo; g.c_obs = dd + o_co; g.shift = dd + o_sh; g.n_obs = dd + o_n;
    g.n_chunks_q = n_chunks_q;
    g.n_chunks_c = n_chunks_c;
    g.partial = (double*)ctx->gof_partial.ptr;
    return SIMPLYP_OK;
}

static void gof_info(const GofSetup& u, int E, simplyp_gof_info* info)
{
    info->n_q_days = (int32_t)u.L.q_day.size();
    info->n_chem_days = (int32_t)u.L.c_day.size();
    info->bytes_read = ((int64_t)u.L.q_day.size() * 8 + (int64_t)u.L.c_day.size() * 32) * E;
    info->n_chunks_q = u.g.n_chunks_q;
    info->n_chunks_chem = u.g.n_chunks_c;
}

static int gof_impl(const Entry& e, const simplyp_dims* dims, uint32_t out_mask,
                    const int32_t* out_reaches, int32_t n_out_reaches,
                    const double* out, const int32_t* member_of_slot,
                    const double* f_tdp, const double* reach_params,
                    const double* obs, double* gof, simplyp_gof_info* info, bool waterbody = false)
{
    simplyp_ctx* const ctx = e.ctx;
    TableView t;
    const bool ptrs_ok = out && f_tdp && (waterbody || reach_params) && obs && gof;
    if (int rc = check_table(e, dims, out_mask, out_reaches, n_out_reaches, ptrs_ok, waterbody, t)) return rc;
    if (info) *info = {};
    constexpr int NV = SIMPLYP_N_GOF_VARS;
    GofSetup u;
    if (int rc = gof_setup(e, t, out, member_of_slot, f_tdp, reach_params, obs, waterbody, simplyp::GOF_NACC,
                           (const void*)simplyp::simplyp_gof_partial_kernel<0>, (const void*)simplyp::simplyp_gof_partial_kernel<1>, u))
        return rc;
    simplyp::GofArgs& g = u.g;
    g.gof = gof;
    const int groups = u.groups, R = t.R;

    if (int rc = e.begin()) return rc;
    hipLaunchKernelGGL(simplyp::simplyp_gof_partial_kernel<0>, dim3(groups, g.n_chunks_q, R), dim3(simplyp::WAVE), 0, ctx->stream, g);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(simplyp::simplyp_gof_partial_kernel<1>, dim3(groups, g.n_chunks_c, R), dim3(simplyp::WAVE), 0, ctx->stream, g);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(simplyp::simplyp_gof_finish_kernel, dim3(groups, R, NV), dim3(simplyp::WAVE), 0, ctx->stream, g);
    if (int rc = e.end(info ? &info->kernel_ms : nullptr)) return rc;
    if (info) gof_info(u, t.E, info);
    return SIMPLYP_OK;
}

// The lag-one sums (simplyp_gof_lag.hip.h): simplyp_gof's setup with four running sums per variable and its own kernels.
int simplyp_gof_lag(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                    const int32_t* out_reaches, int32_t n_out_reaches,
                    const double* out, const int32_t* member_of_slot,
                    const double* f_tdp, const double* reach_params,
                    const double* obs, double* lag, simplyp_gof_info* info)
{
    return entry(ctx, "simplyp_gof_lag", [&](const Entry& e) -> int {
        TableView t;
        const bool ptrs_ok = out && f_tdp && reach_params && obs && lag;
        if (int rc = check_table(e, dims, out_mask, out_reaches, n_out_reaches, ptrs_ok, false, t)) return rc;
        if (info) *info = {};
        constexpr int NV = SIMPLYP_N_GOF_VARS;
        GofSetup u;
        if (int rc = gof_setup(e, t, out, member_of_slot, f_tdp, reach_params, obs, false, simplyp::LAG_NACC,
                               (const void*)simplyp::simplyp_gof_lag_partial_kernel<0>,
                               (const void*)simplyp::simplyp_gof_lag_partial_kernel<1>, u))
            return rc;
        simplyp::GofLagArgs a{};
        a.g = u.g; a.q_succ = u.d_q_succ; a.c_succ = u.d_c_succ; a.lag = lag;
        const int groups = u.groups, R = t.R;
        if (int rc = e.begin()) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_gof_lag_partial_kernel<0>, dim3(groups, a.g.n_chunks_q, R), dim3(simplyp::WAVE), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::simplyp_gof_lag_partial_kernel<1>, dim3(groups, a.g.n_chunks_c, R), dim3(simplyp::WAVE), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::simplyp_gof_lag_finish_kernel, dim3(groups, R, NV), dim3(simplyp::WAVE), 0, ctx->stream, a);
        if (int rc = e.end(info ? &info->kernel_ms : nullptr)) return rc;
        if (info) {
            gof_info(u, t.E, info);
            // the rows a slice re-reads: its first entry continues a segment (the kernels' slice bounds)
            auto rereads = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& succ, int n_chunks) {
                int64_t n = 0;
                for (int r = 0; r < R; ++r)
                    for (int c = 0; c < n_chunks; ++c) {
                        const long long k0 = ptr[r], len = ptr[r + 1] - k0;
                        const long long kb = k0 + len * c / n_chunks, ke = k0 + len * (c + 1) / n_chunks;
                        if (kb < ke && succ[(size_t)kb]) ++n;
                    }
                return n;
            };
            info->bytes_read += (rereads(u.L.q_ptr, u.L.q_succ, a.g.n_chunks_q) * 8 + rereads(u.L.c_ptr, u.L.c_succ, a.g.n_chunks_c) * 32) * t.E;
        }
        return SIMPLYP_OK;
    });
}

int simplyp_gof(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                const int32_t* out_reaches, int32_t n_out_reaches,
                const double* out, const int32_t* member_of_slot,
                const double* f_tdp, const double* reach_params,
                const double* obs, double* gof, simplyp_gof_info* info)
{
    return entry(ctx, "simplyp_gof", [&](const Entry& e) {
        return gof_impl(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, f_tdp, reach_params, obs, gof, info);
    });
}

// Spearman's r per member, variable and output reach (the one column of the reference's table that simplyp_gof leaves out).
int simplyp_gof_spearman(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                         const int32_t* out_reaches, int32_t n_out_reaches,
                         const double* out, const int32_t* member_of_slot,
                         const double* f_tdp, const double* reach_params,
                         const double* obs, double* rho, simplyp_gof_info* info)
{
    return entry(ctx, "simplyp_gof_spearman", [&](const Entry& e) -> int {
        TableView t;
        const bool ptrs_ok = out && f_tdp && reach_params && obs && rho;
        if (int rc = check_table(e, dims, out_mask, out_reaches, n_out_reaches, ptrs_ok, false, t)) return rc;
        const int E = t.E, S = t.S, D = t.D, R = t.R;
        if (info) *info = {};
        constexpr int NV = SIMPLYP_N_GOF_VARS;
        {   // variables without (enough) observations stay NaN (visualise_results.py:430, :453)
            std::vector<double> nanv((size_t)NV * R * E, std::nan(""));
            HIP_TRY(ctx, hipMemcpyAsync(rho, nanv.data(), nanv.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        simplyp::SpearmanArgs g{};
        std::copy(t.col, t.col + 4, g.col);
        g.E = E; g.R = R; g.D = D;
        g.out = out; g.col_stride = (long long)D * R * E;
        g.member_of_slot = member_of_slot; g.f_tdp = f_tdp; g.rho = rho;
        const int groups = (int)blocks(E, simplyp::WAVE);
        double ms_total = 0.0;
        long long pairs = 0;
        int n_q = 0, n_c = 0;
        for (int r = 0; r < R; ++r) {
            for (int v = 0; v < NV; ++v) {
                const double* ob = obs + ((size_t)r * NV + v) * D;
                std::vector<int32_t> day;
                std::vector<double> val;
                for (int d = 0; d < D; ++d) if (ob[d] == ob[d]) { day.push_back(d); val.push_back(ob[d]); }
                const int n = (int)day.size();
                if (n <= 10) continue;                                                    // :430
                // average ranks of the observations (ties share the mean of their positions, like pandas' rank())
                std::vector<int> idx((size_t)n);
                std::iota(idx.begin(), idx.end(), 0);
                std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return val[a] < val[b]; });
                std::vector<double> rk((size_t)n);
                double sum_ro = 0.0, sum_ro2 = 0.0;
                for (int i = 0; i < n;) {
                    int j = i;
                    while (j + 1 < n && val[idx[j + 1]] == val[idx[i]]) ++j;
                    const double avg = 0.5 * ((double)(i + 1) + (double)(j + 1));
                    for (int k = i; k <= j; ++k) rk[idx[k]] = avg;
                    i = j + 1;
                }
                for (int i = 0; i < n; ++i) { sum_ro += rk[i]; sum_ro2 += rk[i] * rk[i]; }
                const int n_blocks = (int)blocks(n, simplyp::SP_TI);
                const size_t list_bytes = ((size_t)n * sizeof(int32_t) + 7) / 8 * 8;
                if (int rc = ensure(ctx, ctx->gof_lists, list_bytes + (size_t)n * sizeof(double))) return rc;
                if (int rc = ensure(ctx, ctx->gof_partial, ((size_t)n + (size_t)n_blocks * 3) * E * sizeof(double))) return rc;
                char* base = (char*)ctx->gof_lists.ptr;
                HIP_TRY(ctx, hipMemcpyAsync(base, day.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(base + list_bytes, rk.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));        // the host vectors go out of scope at the end of this iteration
                g.n = n; g.var = v; g.r = r;
                g.a_catch = reach_params + ((size_t)SIMPLYP_PR_A_CATCH * S + t.reach_of[r]) * E;
                g.day = (const int32_t*)base; g.rank_obs = (const double*)(base + list_bytes);
                g.sum_ro = sum_ro; g.sum_ro2 = sum_ro2;
                g.vals = (double*)ctx->gof_partial.ptr; g.partial = g.vals + (size_t)n * E; g.n_blocks = n_blocks;
                if (int rc = e.begin()) return rc;
                hipLaunchKernelGGL(simplyp::simplyp_spearman_fill_kernel, dim3(groups, (unsigned)std::min(n, 64)), dim3(simplyp::WAVE), 0, ctx->stream, g);
                HIP_TRY(ctx, hipGetLastError());
                hipLaunchKernelGGL(simplyp::simplyp_spearman_count_kernel, dim3(groups, (unsigned)n_blocks), dim3(simplyp::WAVE), 0, ctx->stream, g);
                HIP_TRY(ctx, hipGetLastError());
                hipLaunchKernelGGL(simplyp::simplyp_spearman_finish_kernel, dim3(groups), dim3(simplyp::WAVE), 0, ctx->stream, g);
                double ms = 0.0;
                if (int rc = e.end(&ms)) return rc;
                ms_total += ms;
                pairs += (long long)n * n;
                if (v == SIMPLYP_GOF_Q) n_q += n; else n_c += n;
            }
        }
        if (info) {
            info->kernel_ms = ms_total;
            info->n_q_days = n_q; info->n_chem_days = n_c;
            info->bytes_read = pairs / simplyp::SP_TI * 8 * E;       // rows of the compact table streamed past each block of SP_TI values
        }
        return SIMPLYP_OK;
    });
}

int simplyp_gof_waterbody(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t wb_mask, const double* wb,
                          const int32_t* member_of_slot, const double* f_tdp,
                          const double* obs, double* gof, simplyp_gof_info* info)
{
    return entry(ctx, "simplyp_gof_waterbody", [&](const Entry& e) {
        return gof_impl(e, dims, wb_mask, nullptr, 1, wb, member_of_slot, f_tdp, nullptr, obs, gof, info, true);
    });
}

int simplyp_waterbody(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                      const int32_t* out_reaches, int32_t n_out_reaches,
                      const double* out, const int32_t* member_of_slot,
                      const double* f_tdp, const double* reach_params,
                      const int32_t* sum_reaches, int32_t n_sum,
                      uint32_t wb_mask, double* wb, simplyp_wb_info* info)
{
    return entry(ctx, "simplyp_waterbody", [&](const Entry& e) -> int {
        TableView t;
        const bool ptrs_ok = out && f_tdp && reach_params && sum_reaches && wb;
        if (int rc = check_table(e, dims, out_mask, out_reaches, n_out_reaches, ptrs_ok, false, t)) return rc;
        const int E = t.E, S = t.S, D = t.D, R = t.R;
        if ((wb_mask & SIMPLYP_WB_MASK_ALL) == 0u || (wb_mask & ~SIMPLYP_WB_MASK_ALL) != 0u)
            return e.refuse("wb_mask must select 1..%d of the waterbody columns", (int)SIMPLYP_N_WB);
        if (n_sum < 1 || n_sum > simplyp::WB_MAX_REACHES)
            return e.refuse("n_sum must be in [1, %d] (got %d)", simplyp::WB_MAX_REACHES, n_sum);
        simplyp::WaterbodyArgs g{};
        for (int k = 0; k < n_sum; ++k) {
            const int s = sum_reaches[k];
            if (s < 0 || s >= S) return e.refuse("sum_reaches[%d] = %d out of range", k, s);
            if (k > 0 && s <= sum_reaches[k - 1]) return e.refuse("sum_reaches must be strictly ascending");
            int pos = -1;
            for (int r = 0; r < R; ++r) if (t.reach_of[r] == s) pos = r;
            if (pos < 0) return e.refuse("reach %d is not among the table's output reaches", s);
            g.pos[k] = pos; g.reach[k] = s;
        }
        if (info) *info = {};
        std::copy(t.col, t.col + 4, g.col);
        g.E = E; g.R = R; g.D = D;
        g.out = out; g.col_stride = (long long)D * R * E;
        g.n_sum = n_sum;
        g.member_of_slot = member_of_slot; g.f_tdp = f_tdp;
        g.a_catch = reach_params + (size_t)SIMPLYP_PR_A_CATCH * S * E;
        g.wb_mask = wb_mask; g.wb = wb;
        if (int rc = e.begin()) return rc;
        // two member slots per lane (16-byte accesses) when every row of the tables starts 16-byte aligned
        const bool vec2 = (E % 2 == 0) && (((uintptr_t)out | (uintptr_t)wb) % 16 == 0);
        if (vec2) hipLaunchKernelGGL(simplyp::simplyp_waterbody_kernel<2>, dim3(blocks(E / 2, 256), (unsigned)D), dim3(256), 0, ctx->stream, g);
        else hipLaunchKernelGGL(simplyp::simplyp_waterbody_kernel<1>, dim3(blocks(E, 256), (unsigned)D), dim3(256), 0, ctx->stream, g);
        if (int rc = e.end(info ? &info->kernel_ms : nullptr)) return rc;
        if (info) info->bytes_moved = (int64_t)E * D * (32LL * n_sum + 8LL * popcount32(wb_mask));
        return SIMPLYP_OK;
    });
}

// What a selection across the members decides once per call, whatever it then selects from: the include mask in the table's
// column order and the members that take part (context workspace: 2 x int32 | [E] uint8), and numpy's 'linear' ranks.
// Fills g.E, g.include_slot, g.T, g.rank and g.n_passes (the int before it holds n_used); rank stays unset when n_used == 0.
static int quantile_prepare(simplyp_ctx* ctx, int32_t E, const int32_t* member_of_slot, const uint8_t* include,
                            const double* q, int32_t K, simplyp::QuantileArgs& g, int& n_used)
{
    if (int rc = ensure(ctx, ctx->quant, 16 + (size_t)E)) return rc;
    int* d_ints = (int*)ctx->quant.ptr;                       // [0] members used, [1] sweeps
    uint8_t* d_mask = (uint8_t*)ctx->quant.ptr + 16;
    HIP_TRY(ctx, hipMemsetAsync(d_ints, 0, 16, ctx->stream));
    n_used = E;
    if (include) {
        hipLaunchKernelGGL(simplyp::quantile_mask_kernel, dim3(1), dim3(1024), 0, ctx->stream, (int)E, include, member_of_slot, d_mask, d_ints);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&n_used, d_ints, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    g.E = E; g.include_slot = include ? d_mask : nullptr;
    g.T = 2 * K; g.n_passes = d_ints + 1;
    for (int k = 0; k < K && n_used > 0; ++k) st::linear_ranks(q[k], n_used, g.rank[2 * k], g.rank[2 * k + 1]);
    return SIMPLYP_OK;
}

// The selection of g.n_rows rows of g.table into rows g.out_row0... of g.order_stats: the LDS sort for rows of up to `sort_max`
// members, the radix select for longer ones.
extern "C++" {
template <class Args>
static int select_launch(const Entry& e, const Args& g, int sort_max, void (*sort)(Args, int), void (*select)(Args))
{
    simplyp_ctx* const ctx = e.ctx;
    if (g.E <= sort_max) {
        int P = 2;
        while (P < g.E) P <<= 1;
        const long long rows_per_block = sort_max / P;
        const long long n_blocks = (g.n_rows + rows_per_block - 1) / rows_per_block;
        if (n_blocks > 0x7FFFFFFFLL) return e.refuse("too many rows for one call (%lld)", g.n_rows);
        hipLaunchKernelGGL(sort, dim3((unsigned)n_blocks), dim3(simplyp::QSORT_THREADS), 0, ctx->stream, g, P);
    } else {
        const unsigned n_blocks = (unsigned)std::min<long long>(g.n_rows, 65536);
        hipLaunchKernelGGL(select, dim3(n_blocks), dim3(simplyp::QSEL_THREADS), 0, ctx->stream, g);
    }
    return e.launched();
}

static int select_launch(const Entry& e, const simplyp::QuantileArgs& g)
{
    return select_launch(e, g, simplyp::QSORT_MAX, simplyp::quantile_sort_kernel, simplyp::quantile_select_kernel);
}

static int select_launch(const Entry& e, const simplyp::WQuantileArgs& g)
{
    return select_launch(e, g, simplyp::WQSORT_MAX, simplyp::weighted_sort_kernel, simplyp::weighted_select_kernel);
}
}  // extern "C++"

int simplyp_quantiles(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table,
                      const int32_t* member_of_slot, const uint8_t* include,
                      const double* q, int32_t K, double* order_stats, simplyp_quantile_info* info)
{
    return entry(ctx, "simplyp_quantiles", [&](const Entry& e) -> int {
        if (E < 1 || n_rows < 0)
            return e.refuse("E must be >= 1 and n_rows >= 0 (got E = %d, n_rows = %lld)", (int)E, (long long)n_rows);
        if (!table || !q || !order_stats) return e.refuse("table, q and order_stats must not be NULL");
        TABLE_TRY(ctx, st::check_probabilities(e.me, q, K, simplyp::QUANT_MAX_K, msg));
        if (info) { *info = {}; info->bytes_table = n_rows * (int64_t)E * 8; }
        if (n_rows == 0) return SIMPLYP_OK;
        if (int rc = e.begin()) return rc;
        simplyp::QuantileArgs g{};
        int n_used = 0;
        if (int rc = quantile_prepare(ctx, E, member_of_slot, include, q, K, g, n_used)) return rc;
        const long long n_out = 2LL * K * n_rows;
        if (n_used == 0) {
            if (int rc = fill_nan(e, order_stats, n_out)) return rc;
        } else {
            g.n_rows = n_rows; g.table = table; g.order_stats = order_stats; g.out_row0 = 0; g.out_stride = n_rows;
            if (int rc = select_launch(e, g)) return rc;
        }
        int n_passes = 0;
        if (int rc = e.end(info ? &info->kernel_ms : nullptr, &n_passes, g.n_passes, sizeof(int))) return rc;
        if (info) { info->n_used = n_used; info->n_passes = n_passes; }
        return SIMPLYP_OK;
    });
}

// ---- weighted bands (simplyp_weighted.h states the rule, simplyp_quantile.hip.h selects) --------------------------------------
// What a weighted selection decides once per call: the weights in the table's column order, their sum, who takes part
// (context workspace: WqPrepared | [E] uint64) and, from the sum read back, every probability's exact threshold.  Fills g.E,
// g.w_slot, g.K, g.thr and g.n_passes; thr stays unset when T == 0.  A weight above 2^40 is SIMPLYP_ERR_ARG.
static int weighted_prepare(const Entry& e, int32_t E, const int32_t* member_of_slot, const uint8_t* include,
                            const uint64_t* weights, const double* q, int32_t K, simplyp::WQuantileArgs& g, simplyp::WqPrepared& got)
{
    simplyp_ctx* const ctx = e.ctx;
    if (int rc = ensure(ctx, ctx->wquant, sizeof(simplyp::WqPrepared) + (size_t)E * sizeof(uint64_t))) return rc;
    simplyp::WqPrepared* d_res = (simplyp::WqPrepared*)ctx->wquant.ptr;
    unsigned long long* d_w = (unsigned long long*)((char*)ctx->wquant.ptr + sizeof(simplyp::WqPrepared));
    hipLaunchKernelGGL(simplyp::weighted_prepare_kernel, dim3(1), dim3(1024), 0, ctx->stream, (int)E, (const unsigned long long*)weights,
                       include, member_of_slot, d_w, d_res);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&got, d_res, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    TABLE_TRY(ctx, simplyp_weighted::check_weights(e.me, got.n_bad, msg));
    g.E = E; g.w_slot = d_w; g.K = K; g.n_passes = &d_res->n_passes;
    for (int k = 0; k < K && got.T > 0; ++k) g.thr[k] = simplyp_weighted::weighted_threshold(q[k], got.T);
    return SIMPLYP_OK;
}

int simplyp_weighted_quantiles(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table,
                               const int32_t* member_of_slot, const uint8_t* include, const uint64_t* weights,
                               const double* q, int32_t K, double* order_stats, simplyp_wq_info* info)
{
    return entry(ctx, "simplyp_weighted_quantiles", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, simplyp_weighted::check_table(e.me, E, n_rows, table, weights, q, K, order_stats, msg));
        if (info) { *info = {}; info->bytes_table = n_rows * (int64_t)E * 8; }
        if (n_rows == 0) return SIMPLYP_OK;
        if (int rc = e.begin()) return rc;
        simplyp::WQuantileArgs g{};
        simplyp::WqPrepared got{};
        if (int rc = weighted_prepare(e, E, member_of_slot, include, weights, q, K, g, got)) return rc;
        if (got.T == 0) {
            if (int rc = fill_nan(e, order_stats, (long long)K * n_rows)) return rc;
        } else {
            g.n_rows = n_rows; g.table = table; g.order_stats = order_stats; g.out_row0 = 0; g.out_stride = n_rows;
            if (int rc = select_launch(e, g)) return rc;
        }
        int n_passes = 0;
        if (int rc = e.end(info ? &info->kernel_ms : nullptr, &n_passes, g.n_passes, sizeof(int))) return rc;
        if (info) { info->T = got.T; info->n_used = got.n_used; info->n_passes = n_passes; }
        return SIMPLYP_OK;
    });
}

int simplyp_time_quantiles(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                           const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                           const double* f_tdp, const double* reach_params,
                           const int32_t* series, int32_t n_series, const int32_t* period_of_day, int32_t n_periods,
                           const double* q, int32_t K, double* order_stats, int32_t* n_days, simplyp_tq_info* info)
{
    return entry(ctx, "simplyp_time_quantiles", [&](const Entry& e) -> int {
        if (!dims || dims->E < 1 || dims->S < 1 || dims->D < 0)
            return e.refuse("bad dims (E and S must be >= 1, D >= 0)");
        if (!out || !q || !order_stats) return e.refuse("out, q and order_stats must not be NULL");
        TABLE_TRY(ctx, st::check_probabilities(e.me, q, K, simplyp::TQ_MAX_K, msg));
        st::View tab;
        TABLE_TRY(ctx, st::view(e.me, *dims, out_mask, st::DAILY_COLUMNS, out_reaches, n_out_reaches, tab, msg));
        const int E = tab.E, S = tab.S, D = tab.D, R = tab.R;
        st::Series sr;
        simplyp::TqArgs g{};
        TABLE_TRY(ctx, st::resolve_series(e.me, series, n_series, simplyp::TQ_MAX_SERIES, out_mask, R, f_tdp, reach_params, g.series, nullptr, sr, msg));
        if (n_periods < 0 || (!period_of_day && n_periods > 1) || (period_of_day && n_periods < 1))
            return e.refuse("period_of_day needs n_periods >= 1; without it n_periods is 0 (or 1)");
        const int P = std::max<int>(n_periods, 1);
        std::vector<int32_t> day_ptr, days;
        TABLE_TRY(ctx, st::period_days(e.me, period_of_day, D, P, days, day_ptr, msg));
        if (n_days) for (int p = 0; p < P; ++p) n_days[p] = day_ptr[p + 1] - day_ptr[p];
        if (info) { *info = {}; info->n_periods = P; }

        // ranks per period: k_lo, k_hi of every probability, ascending without repeats (rows padded with their last rank)
        const int T = 2 * K;
        std::vector<int32_t> ranks((size_t)P * T, 0);
        std::vector<uint8_t> rank_of((size_t)P * T, 0);
        for (int p = 0; p < P; ++p) {
            const long long n = day_ptr[p + 1] - day_ptr[p];
            if (n <= 0) continue;
            long long want[2 * simplyp::TQ_MAX_K];
            for (int k = 0; k < K; ++k) st::linear_ranks(q[k], n, want[k], want[K + k]);
            std::vector<long long> u(want, want + T);
            std::sort(u.begin(), u.end());
            u.erase(std::unique(u.begin(), u.end()), u.end());
            for (int t = 0; t < T; ++t) ranks[(size_t)p * T + t] = (int32_t)u[std::min<size_t>(t, u.size() - 1)];
            for (int k = 0; k < T; ++k)
                rank_of[(size_t)p * T + k] = (uint8_t)(std::lower_bound(u.begin(), u.end(), want[k]) - u.begin());
        }

        const long long n_out = 2LL * K * n_series * P * R * E;
        if (days.empty()) {                                        // no day takes part in any period (D = 0 among them): all NaN
            if (int rc = fill_nan(e, order_stats, n_out)) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return SIMPLYP_OK;
        }
        // device workspace: 16 bytes of counters, then the int32 lists and the byte map -- O(D K), whatever E and the table's size
        Staging up;
        const size_t o_day = up.put(days), o_ptr = up.put(day_ptr), o_ranks = up.put(ranks), o_reach = up.put(tab.reach_of);
        const size_t int_bytes = up.bytes();
        if (int rc = ensure(ctx, ctx->tquant, 16 + int_bytes + rank_of.size())) return rc;
        char* base = (char*)ctx->tquant.ptr;
        HIP_TRY(ctx, hipMemsetAsync(base, 0, 16, ctx->stream));
        if (int rc = up.upload(e, base + 16)) return rc;
        const int32_t* d_ints = up.d_ints;
        HIP_TRY(ctx, hipMemcpyAsync(base + 16 + int_bytes, rank_of.data(), rank_of.size(), hipMemcpyHostToDevice, ctx->stream));

        g.E = E; g.R = R; g.D = D; g.K = K; g.T = T; g.n_series = n_series; g.n_periods = P;
        g.out = out; g.col_stride = (long long)D * R * E;
        st::flux_slots(out_mask, st::FLUX_COLS, g.col);
        g.member_of_slot = member_of_slot;
        g.f_tdp = f_tdp;
        g.a_catch = sr.derived ? reach_params + (size_t)SIMPLYP_PR_A_CATCH * S * E : nullptr;
        g.day = d_ints + o_day; g.day_ptr = d_ints + o_ptr; g.ranks = d_ints + o_ranks; g.reach_of = d_ints + o_reach;
        g.rank_of = (const uint8_t*)(base + 16 + int_bytes);
        g.order_stats = order_stats;
        g.rows_read = (unsigned long long*)base;
        g.n_sweeps = (int*)(base + 8);
        const dim3 grid(blocks(E, 64), (unsigned)std::min(P, 65535), (unsigned)(n_series * R));
        if (int rc = e.begin()) return rc;
        // the per-rank state of 8 ranks (K <= 4) leaves room for two workgroups' histograms per CU; 32 ranks for one
        if (T <= 8) hipLaunchKernelGGL(simplyp::simplyp_time_quantile_kernel<8>, grid, dim3(64), 0, ctx->stream, g);
        else hipLaunchKernelGGL(simplyp::simplyp_time_quantile_kernel<32>, grid, dim3(64), 0, ctx->stream, g);
        unsigned long long counters[2] = {0ull, 0ull};
        if (int rc = e.end(info ? &info->kernel_ms : nullptr, counters, base, 16)) return rc;
        if (info) {
            info->bytes_read = (int64_t)(counters[0] * 512ull);
            info->n_sweeps = (int32_t)(counters[1] & 0xFFFFFFFFull);
        }
        return SIMPLYP_OK;
    });
}

// What simplyp_predictive_series and simplyp_predictive_bands share: the checks of the table and the series, and the
// generation kernel's arguments but for the block of days and its destination.  reach_bytes: the room the device copy of the
// output reaches takes at the head of ctx->pred.
static int predictive_setup(const Entry& e, const simplyp_dims* dims, uint32_t out_mask,
                            const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                            const double* f_tdp, const double* reach_params, const int32_t* series, int32_t n_series,
                            const double* err_m, uint64_t seed, int32_t day0, simplyp::PredArgs& g, st::View& t, st::Series& sr)
{
    simplyp_ctx* const ctx = e.ctx;
    if (!dims || dims->E < 1 || dims->S < 1 || dims->D < 0)
        return e.refuse("bad dims (E and S must be >= 1, D >= 0: the table's daily rows)");
    if (!out) return e.refuse("out must not be NULL");
    if (day0 < 0 || (long long)day0 + dims->D > 0x7FFFFFFFLL)
        return e.refuse("day0 must be >= 0 and day0 + D fit 31 bits (got %d)", (int)day0);
    TABLE_TRY(ctx, st::view(e.me, *dims, out_mask, st::DAILY_COLUMNS, out_reaches, n_out_reaches, t, msg));
    const int E = t.E, S = t.S, D = t.D, R = t.R;
    TABLE_TRY(ctx, st::resolve_series(e.me, series, n_series, simplyp::PRED_MAX_SERIES, out_mask, R, f_tdp, reach_params, g.series, g.series_id, sr, msg));
    g.E = E; g.R = R; g.n_series = n_series;
    g.out = out; g.col_stride = (long long)D * R * E;
    st::flux_slots(out_mask, st::FLUX_COLS, g.col);
    g.member_of_slot = member_of_slot;
    g.f_tdp = f_tdp;
    g.a_catch = sr.derived ? reach_params + (size_t)SIMPLYP_PR_A_CATCH * S * E : nullptr;
    g.err_m = err_m;
    philox_key(seed, g);
    g.day0 = (uint32_t)day0;
    return SIMPLYP_OK;
}

constexpr size_t PRED_REACH_BYTES = 4 * 65536;      // n_out_reaches <= 65535

// The output reaches to the head of ctx->pred (grown to hold `table_bytes` behind them).
static int predictive_workspace(simplyp_ctx* ctx, const std::vector<int32_t>& reach_of, size_t table_bytes, simplyp::PredArgs& g)
{
    if (int rc = ensure(ctx, ctx->pred, PRED_REACH_BYTES + table_bytes)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pred.ptr, reach_of.data(), reach_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    g.reach_of = (const int32_t*)ctx->pred.ptr;
    return SIMPLYP_OK;
}

static int predictive_launch(simplyp_ctx* ctx, simplyp::PredArgs& g, int d_lo, int n_days, double* dst)
{
    g.d_lo = d_lo; g.n_days = n_days; g.dst = dst;
    const int batches = (int)blocks(n_days, simplyp::PRED_BATCH);
    const dim3 grid(blocks(g.E, simplyp::PRED_THREADS), (unsigned)std::min(batches, 65535), (unsigned)(g.n_series * g.R));
    hipLaunchKernelGGL(simplyp::simplyp_predictive_kernel, grid, dim3(simplyp::PRED_THREADS), 0, ctx->stream, g);
    HIP_TRY(ctx, hipGetLastError());
    return SIMPLYP_OK;
}

int simplyp_predictive_series(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                              const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                              const double* f_tdp, const double* reach_params, const int32_t* series, int32_t n_series,
                              const double* err_m, uint64_t seed, int32_t day0, int32_t which, double* table)
{
    return entry(ctx, "simplyp_predictive_series", [&](const Entry& e) -> int {
        if (which < 0 || which > 1) return e.refuse("which must be 0 (values) or 1 (normals), got %d", (int)which);
        if (which == 1 && !err_m) return e.refuse("which = 1 (the normals) needs err_m");
        if (!table) return e.refuse("table must not be NULL");
        simplyp::PredArgs g{};
        st::View t;
        st::Series sr;
        if (int rc = predictive_setup(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, f_tdp, reach_params,
                                      series, n_series, err_m, seed, day0, g, t, sr)) return rc;
        if (dims->D == 0) return SIMPLYP_OK;
        if (int rc = predictive_workspace(ctx, t.reach_of, 0, g)) return rc;
        g.normals = which;
        if (int rc = predictive_launch(ctx, g, 0, dims->D, table)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return SIMPLYP_OK;
    });
}

namespace {
// What the bands select every chunk with: either selection, prepared once per call.
struct BandSelection {
    std::variant<simplyp::QuantileArgs, simplyp::WQuantileArgs> args;
    simplyp::WqPrepared got{};             // under weights: their sum and the members that carry one
    int n_used = 0;                        // members that take part; 0: every value of the result is NaN
    int T = 0;                             // planes of the result: 2K, K under weights
    simplyp::SelectArgs& head() { return std::visit([](auto& a) -> simplyp::SelectArgs& { return a; }, args); }
    void set_rows(const double* table, long long n_rows, long long out_row0)
    {
        simplyp::SelectArgs& h = head();
        h.table = table; h.n_rows = n_rows; h.out_row0 = out_row0;
    }
    int launch(const Entry& e) { return std::visit([&](auto& a) { return select_launch(e, a); }, args); }
};
}  // namespace

static int predictive_bands_impl(const Entry& e, const simplyp_dims* dims, uint32_t out_mask,
                                 const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                                 const uint8_t* include, const double* f_tdp, const double* reach_params,
                                 const int32_t* series, int32_t n_series, const double* err_m, uint64_t seed, int32_t day0,
                                 const double* q, int32_t K, double* order_stats, simplyp_pred_info* info,
                                 bool weighted = false, const uint64_t* weights = nullptr, simplyp_wq_info* winfo = nullptr)
{
    // `weighted`: simplyp_predictive_bands_weighted -- the same generation, chunks and checks; one plane of values selected under
    // `weights` by the weighted selectors, and `winfo` instead of `info`
    simplyp_ctx* const ctx = e.ctx;
    if (weighted) {
        TABLE_TRY(ctx, simplyp_weighted::check_selection(e.me, dims ? dims->E : 1, weights, q, K, order_stats, msg));
    } else {
        if (!q || !order_stats) return e.refuse("q and order_stats must not be NULL");
        TABLE_TRY(ctx, st::check_probabilities(e.me, q, K, simplyp::QUANT_MAX_K, msg));
    }
    simplyp::PredArgs g{};
    st::View t;
    st::Series sr;
    if (int rc = predictive_setup(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, f_tdp, reach_params,
                                  series, n_series, err_m, seed, day0, g, t, sr)) return rc;
    const int E = g.E, R = g.R, D = dims->D;
    if (info) *info = {};
    if (winfo) { *winfo = {}; winfo->bytes_table = (int64_t)n_series * D * R * E * 8; }
    if (D == 0) return SIMPLYP_OK;
    // whole days per chunk: what 256 MiB of generated series hold, or what the environment says
    const size_t day_bytes = (size_t)n_series * R * E * sizeof(double);
    long long chunk_days = std::max<long long>(1, (long long)((256ull << 20) / day_bytes));
    if (const char* env = std::getenv("SIMPLYP_PRED_CHUNK_DAYS")) {
        const long long v = std::atoll(env);
        if (v > 0) chunk_days = v;
    }
    chunk_days = std::min<long long>(chunk_days, D);
    const int n_chunks = (int)((D + chunk_days - 1) / chunk_days);
    const hipEvent_t gen_from = ctx->ev_lap[0], gen_to = ctx->ev_lap[1];
    if (int rc = predictive_workspace(ctx, t.reach_of, (size_t)chunk_days * day_bytes, g)) return rc;
    double* work = (double*)((char*)ctx->pred.ptr + PRED_REACH_BYTES);
    if (int rc = e.begin()) return rc;
    BandSelection sel;
    if (weighted) {                                                                                   // once per call
        if (int rc = weighted_prepare(e, E, member_of_slot, include, weights, q, K, sel.args.emplace<simplyp::WQuantileArgs>(), sel.got)) return rc;
        sel.n_used = sel.got.T > 0 ? sel.got.n_used : 0;
        sel.T = K;
    } else {
        if (int rc = quantile_prepare(ctx, E, member_of_slot, include, q, K, sel.args.emplace<simplyp::QuantileArgs>(), sel.n_used)) return rc;
        sel.T = 2 * K;
    }
    const int n_used = sel.n_used;
    const long long n_rows_all = (long long)n_series * D * R;
    double gen_ms = 0.0;
    if (n_used == 0) {
        if (int rc = fill_nan(e, order_stats, (long long)sel.T * n_rows_all)) return rc;
    } else {
        sel.head().order_stats = order_stats; sel.head().out_stride = n_rows_all;
        for (int c = 0; c < n_chunks; ++c) {
            const int d_lo = (int)(c * chunk_days), nd = (int)std::min<long long>(chunk_days, D - d_lo);
            HIP_TRY(ctx, hipEventRecord(gen_from, ctx->stream));
            if (int rc = predictive_launch(ctx, g, d_lo, nd, work)) return rc;
            HIP_TRY(ctx, hipEventRecord(gen_to, ctx->stream));
            for (int i = 0; i < n_series; ++i) {               // a series' rows of the chunk are one run of rows of the result
                sel.set_rows(work + (size_t)i * nd * R * E, (long long)nd * R, ((long long)i * D + d_lo) * R);
                if (int rc = sel.launch(e)) return rc;
            }
            // the generation's time, read while the chunk's selections run; the next chunk overwrites the workspace after them
            HIP_TRY(ctx, hipEventSynchronize(gen_to));
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, gen_from, gen_to));
            gen_ms += ms;
        }
    }
    int n_passes = 0;
    double kernel_ms = 0.0;
    if (int rc = e.end(&kernel_ms, &n_passes, sel.head().n_passes, sizeof(int))) return rc;
    if (winfo) { winfo->kernel_ms = kernel_ms; winfo->T = sel.got.T; winfo->n_used = sel.got.n_used; winfo->n_passes = n_passes; }
    if (info) {
        info->kernel_ms = kernel_ms;
        info->gen_ms = gen_ms;
        info->bytes_read = n_used == 0 ? 0 : sr.loads * (int64_t)D * R * E * 8;
        info->bytes_workspace = (int64_t)((size_t)chunk_days * day_bytes);
        info->n_used = n_used;
        info->n_passes = n_passes;
        info->n_chunks = n_used == 0 ? 0 : n_chunks;
    }
    return SIMPLYP_OK;
}

int simplyp_predictive_bands(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                             const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                             const uint8_t* include, const double* f_tdp, const double* reach_params,
                             const int32_t* series, int32_t n_series, const double* err_m, uint64_t seed, int32_t day0,
                             const double* q, int32_t K, double* order_stats, simplyp_pred_info* info)
{
    return entry(ctx, "simplyp_predictive_bands", [&](const Entry& e) {
        return predictive_bands_impl(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, include, f_tdp, reach_params,
                                     series, n_series, err_m, seed, day0, q, K, order_stats, info);
    });
}

int simplyp_predictive_bands_weighted(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                                      const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                                      const uint8_t* include, const double* f_tdp, const double* reach_params,
                                      const int32_t* series, int32_t n_series, const double* err_m, uint64_t seed, int32_t day0,
                                      const double* q, int32_t K, const uint64_t* weights, double* order_stats, simplyp_wq_info* info)
{
    return entry(ctx, "simplyp_predictive_bands_weighted", [&](const Entry& e) {
        return predictive_bands_impl(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, include, f_tdp, reach_params,
                                     series, n_series, err_m, seed, day0, q, K, order_stats, nullptr, true, weights, info);
    });
}

// ---- scores (simplyp_score.h states the rule, simplyp_score.hip.h holds the kernels) ------------------------------------------
// B's sort of g.n_rows rows into the workspace: the tiles, then the merge passes.  `src`: the buffer that holds the result.
static int score_sort_launch(simplyp_ctx* ctx, const simplyp::ScoreArgs& g, int& src)
{
    const unsigned n_tiles = blocks(g.E, simplyp::SCORE_TILE);
    int P = 2;
    while (P < std::min(g.E, simplyp::SCORE_TILE)) P <<= 1;
    hipLaunchKernelGGL(simplyp::score_tile_sort_kernel, dim3(n_tiles, (unsigned)g.n_rows), dim3(simplyp::SCORE_THREADS), 0, ctx->stream, g, P);
    HIP_TRY(ctx, hipGetLastError());
    src = 0;
    const dim3 grid(blocks(g.E, simplyp::SCORE_THREADS), (unsigned)g.n_rows);
    for (long long L = simplyp::SCORE_TILE; L < g.E; L *= 2, src ^= 1) {
        hipLaunchKernelGGL(simplyp::score_merge_kernel, grid, dim3(simplyp::SCORE_THREADS), 0, ctx->stream, g, (int)L, src);
        HIP_TRY(ctx, hipGetLastError());
    }
    return SIMPLYP_OK;
}

// What simplyp_scores and simplyp_predictive_scores share.  `rows`: the scored rows of the result ([n_rows_all] rows), ascending,
// with their observations `ys`.  table != NULL: row rows[i] of it is scored row i; otherwise `pg` and `rows3` (3 ints per scored
// row: series index, day, output reach) generate the chunk's rows into the workspace first.
static int scores_common(const Entry& e, int32_t E, const int32_t* member_of_slot, const uint8_t* include,
                         const uint64_t* weights, const std::vector<int64_t>& rows, const std::vector<double>& ys, int64_t n_rows_all,
                         const double* table, simplyp::PredArgs* pg, const std::vector<int32_t>& rows3, int64_t loads,
                         double* sums, uint64_t* counts, simplyp_score_info* info)
{
    simplyp_ctx* const ctx = e.ctx;
    const int64_t n_scored = (int64_t)rows.size();
    const bool gen = table == nullptr;
    const uint64_t row_bytes = (uint64_t)E * 8ull * (gen ? 5ull : 4ull);
    int64_t chunk = simplyp_score::chunk_rows(n_scored, row_bytes, 256ull << 20, std::getenv("SIMPLYP_SCORE_CHUNK_ROWS"));
    chunk = std::min<int64_t>(chunk, 65535);
    const size_t ones_bytes = ((size_t)E * 8 + 255) & ~(size_t)255;
    const size_t list_bytes = ((size_t)n_scored * (8 + 8 + 8 + 12) + 255) & ~(size_t)255;
    if (int rc = ensure(ctx, ctx->score, ones_bytes + list_bytes + (n_scored ? (size_t)chunk * row_bytes : 0))) return rc;
    char* base = (char*)ctx->score.ptr;
    if (int rc = e.begin()) return rc;
    const uint64_t* d_weights = weights;
    if (!weights) {
        hipLaunchKernelGGL(simplyp::score_ones_kernel, dim3(blocks(E, 256)), dim3(256), 0, ctx->stream, (unsigned long long*)base, (int)E);
        HIP_TRY(ctx, hipGetLastError());
        d_weights = (const uint64_t*)base;
    }
    simplyp::WQuantileArgs wq{};
    simplyp::WqPrepared got{};
    if (int rc = weighted_prepare(e, E, member_of_slot, include, d_weights, nullptr, 0, wq, got)) return rc;
    // every row starts as "not scored"
    if (int rc = fill_nan(e, sums, 2 * n_rows_all)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)(2 * n_rows_all) * sizeof(uint64_t), ctx->stream));
    double gen_ms = 0.0, sort_ms = 0.0;
    int n_chunks = 0;
    if (got.T > 0 && n_scored > 0) {
        long long* d_dst = (long long*)(base + ones_bytes);
        double* d_y = (double*)(d_dst + n_scored);
        int32_t* d_rows3 = (int32_t*)(d_y + n_scored);
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, rows.data(), (size_t)n_scored * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_y, ys.data(), (size_t)n_scored * 8, hipMemcpyHostToDevice, ctx->stream));
        if (gen) HIP_TRY(ctx, hipMemcpyAsync(d_rows3, rows3.data(), (size_t)n_scored * 12, hipMemcpyHostToDevice, ctx->stream));
        unsigned long long* work = (unsigned long long*)(base + ones_bytes + list_bytes);
        const size_t plane = (size_t)chunk * E;
        simplyp::ScoreArgs g{};
        g.E = E; g.w_slot = wq.w_slot; g.T = got.T;
        g.sums = sums; g.counts = (unsigned long long*)counts; g.out_stride = n_rows_all;
        g.keys[0] = work; g.keys[1] = work + plane; g.wts[0] = work + 2 * plane; g.wts[1] = work + 3 * plane;
        const hipEvent_t* ev = ctx->ev_lap;         // a chunk's start, its rows generated, its rows sorted
        for (int64_t r0 = 0; r0 < n_scored; r0 += chunk, ++n_chunks) {
            g.n_rows = (int)std::min<int64_t>(chunk, n_scored - r0);
            g.y = d_y + r0; g.dst = d_dst + r0;
            HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
            if (gen) {
                pg->dst = (double*)(work + 4 * plane);
                const dim3 grid(blocks(E, simplyp::PRED_THREADS), (unsigned)g.n_rows);
                hipLaunchKernelGGL(simplyp::score_rows_kernel, grid, dim3(simplyp::PRED_THREADS), 0, ctx->stream, *pg,
                                   (const int*)(d_rows3 + 3 * r0), g.n_rows);
                HIP_TRY(ctx, hipGetLastError());
                g.table = pg->dst; g.row = nullptr;
            } else {
                g.table = table; g.row = d_dst + r0;
            }
            HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
            int src = 0;
            if (int rc = score_sort_launch(ctx, g, src)) return rc;
            HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
            hipLaunchKernelGGL(simplyp::score_gap_kernel, dim3((unsigned)g.n_rows), dim3(simplyp::SCORE_THREADS), 0, ctx->stream, g, src);
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(simplyp::score_stream_kernel, dim3((unsigned)g.n_rows), dim3(simplyp::SCORE_THREADS), 0, ctx->stream, g);
            HIP_TRY(ctx, hipGetLastError());
            // the chunk's generation and sort times, read while its sums run; the next chunk overwrites the workspace after them
            HIP_TRY(ctx, hipEventSynchronize(ev[2]));
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
            gen_ms += ms;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[1], ev[2]));
            sort_ms += ms;
        }
    }
    double kernel_ms = 0.0;
    if (int rc = e.end(&kernel_ms)) return rc;
    if (info) {
        info->kernel_ms = kernel_ms; info->gen_ms = gen_ms; info->sort_ms = sort_ms;
        info->bytes_read = got.T > 0 ? loads * n_scored * (int64_t)E * 8 : 0;
        info->bytes_workspace = got.T > 0 && n_scored > 0 ? (int64_t)((uint64_t)chunk * row_bytes) : 0;
        info->T = got.T; info->n_used = got.n_used;
        info->n_rows_scored = got.T > 0 ? (int32_t)n_scored : 0;
        info->n_chunks = n_chunks;
    }
    return SIMPLYP_OK;
}

int simplyp_scores(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table,
                   const int32_t* member_of_slot, const uint8_t* include, const uint64_t* weights,
                   const double* y, double* sums, uint64_t* counts, simplyp_score_info* info)
{
    return entry(ctx, "simplyp_scores", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, simplyp_score::check_table(e.me, E, n_rows, table, y, sums, counts, msg));
        std::vector<int64_t> rows;
        TABLE_TRY(ctx, simplyp_score::scored_rows(e.me, y, n_rows, rows, msg));
        if (info) *info = {};
        if (n_rows == 0) return SIMPLYP_OK;
        std::vector<double> ys(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) ys[i] = y[rows[i]];
        return scores_common(e, E, member_of_slot, include, weights, rows, ys, n_rows, table, nullptr, std::vector<int32_t>(), 1,
                             sums, counts, info);
    });
}

int simplyp_predictive_scores(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                              const int32_t* out_reaches, int32_t n_out_reaches, const double* out, const int32_t* member_of_slot,
                              const uint8_t* include, const double* f_tdp, const double* reach_params,
                              const int32_t* series, int32_t n_series, const double* err_m, uint64_t seed, int32_t day0,
                              const uint64_t* weights, const double* obs, double* sums, uint64_t* counts, simplyp_score_info* info)
{
    return entry(ctx, "simplyp_predictive_scores", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, simplyp_score::check_outputs(e.me, dims ? dims->E : 1, obs, sums, counts, msg));
        simplyp::PredArgs g{};
        st::View t;
        st::Series sr;
        if (int rc = predictive_setup(e, dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, f_tdp, reach_params,
                                      series, n_series, err_m, seed, day0, g, t, sr)) return rc;
        const int R = g.R, D = dims->D;
        const int64_t n_rows_all = (int64_t)n_series * D * R;
        std::vector<int64_t> rows;
        TABLE_TRY(ctx, simplyp_score::scored_rows(e.me, obs, n_rows_all, rows, msg));
        if (info) *info = {};
        if (D == 0) return SIMPLYP_OK;
        std::vector<double> ys(rows.size());
        std::vector<int32_t> rows3(3 * rows.size());
        for (size_t i = 0; i < rows.size(); ++i) {
            ys[i] = obs[rows[i]];
            rows3[3 * i] = (int32_t)(rows[i] / ((int64_t)D * R));
            rows3[3 * i + 1] = (int32_t)((rows[i] / R) % D);
            rows3[3 * i + 2] = (int32_t)(rows[i] % R);
        }
        if (int rc = predictive_workspace(ctx, t.reach_of, 0, g)) return rc;
        return scores_common(e, g.E, member_of_slot, include, weights, rows, ys, n_rows_all, nullptr, &g, rows3, sr.loads,
                             sums, counts, info);
    });
}

// ---- Pareto counts and ranks (simplyp_pareto.h states the rule, simplyp_pareto.hip.h holds the kernels) ------------------------
extern "C++" {
template <int MODE>
static void pareto_pairs_launch(simplyp_ctx* ctx, int M, dim3 grid, const unsigned long long* key, long long stride, int n_i,
                                const int* ilist, int n_j, const int* jlist, int* by_count, int* of_count)
{
    const dim3 block(simplyp::PARETO_THREADS);
#define PARETO_CASE(MP)                                                                                                     \
    hipLaunchKernelGGL((simplyp::pareto_pairs_kernel<MP, MODE>), grid, block, 0, ctx->stream, key, stride, M, n_i, ilist, n_j, jlist, \
                       by_count, of_count)
    switch (M) {                                    // M padded to the next compiled size
    case 1: PARETO_CASE(1); break;
    case 2: PARETO_CASE(2); break;
    case 3: PARETO_CASE(3); break;
    case 4: PARETO_CASE(4); break;
    case 5: case 6: PARETO_CASE(6); break;
    default: PARETO_CASE(8); break;
    }
#undef PARETO_CASE
}
}  // extern "C++"

int simplyp_pareto(simplyp_ctx* ctx, int32_t E, int32_t M, const double* obj, const int32_t* sense, const int32_t* member_of_slot,
                   const uint8_t* include, int32_t max_fronts, int32_t* dominated_by, int32_t* dominates, int32_t* rank,
                   simplyp_pareto_info* info)
{
    return entry(ctx, "simplyp_pareto", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, simplyp_pareto_rules::check_args(e.me, E, M, obj, sense, max_fronts, dominated_by, dominates, rank, msg));
        if (info) *info = {};
        const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const int T = simplyp::PARETO_THREADS;
        const int n_blocks = (int)blocks(E, T);
        const size_t ints = pad((size_t)E * sizeof(int));
        const size_t off_flag = 256, off_sum = off_flag + pad((size_t)E), off_key = off_sum + pad((size_t)n_blocks * sizeof(int));
        const size_t off_ints = off_key + pad((size_t)M * E * sizeof(unsigned long long));
        if (int rc = ensure(ctx, ctx->pareto, off_ints + 8 * ints)) return rc;
        char* base = (char*)ctx->pareto.ptr;
        int* d_head = (int*)base;                       // [0] n, [4..7] the peeling's two pairs of counters
        int* d_int[8];                                  // members, dominated_by, dominates, left, rank, front, alive x 2
        for (int k = 0; k < 8; ++k) d_int[k] = (int*)(base + off_ints + k * ints);
        simplyp::ParetoPrepArgs g{};
        g.E = E; g.M = M; g.n_blocks = n_blocks; g.obj = obj; g.member_of_slot = member_of_slot; g.include = include;
        for (int m = 0; m < M; ++m) g.sense[m] = sense[m];
        g.flag = (uint8_t*)(base + off_flag); g.block_sum = (int*)(base + off_sum); g.n = d_head;
        g.key = (unsigned long long*)(base + off_key); g.member_of = d_int[0];
        if (int rc = e.begin()) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_head, 0, 256, ctx->stream));
        const dim3 block(T), grid_E((unsigned)n_blocks);
        hipLaunchKernelGGL(simplyp::pareto_flag_kernel, grid_E, block, 0, ctx->stream, g);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::pareto_scan_kernel, dim3(1), block, 0, ctx->stream, g);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::pareto_compact_kernel, grid_E, block, 0, ctx->stream, g);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::pareto_fill_kernel, grid_E, block, 0, ctx->stream, (int)E, SIMPLYP_PARETO_EXCLUDED, dominated_by, dominates, rank);
        HIP_TRY(ctx, hipGetLastError());
        int n = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&n, d_head, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (n < 0 || n > E) return fail(ctx, SIMPLYP_ERR_DEVICE, "%s: the prepare kernels count %d participants of %d members", e.me, n, (int)E);
        int64_t pair_tests = 0;
        int n_fronts = 0, n_front0 = 0, n_unranked = 0;
        if (n > 0) {
            const dim3 grid_n(blocks(n, T));
            const unsigned splits = blocks(n, simplyp::PARETO_JSPLIT);
            HIP_TRY(ctx, hipMemsetAsync(d_int[1], 0, 2 * ints, ctx->stream));       // both counts
            const char* how = std::getenv("SIMPLYP_PARETO_JLOAD");                  // "scalar": the j keys from memory, not from LDS
            if (how && std::strcmp(how, "scalar") == 0)
                pareto_pairs_launch<1>(ctx, M, dim3(grid_n.x, splits), g.key, E, n, nullptr, n, nullptr, d_int[1], d_int[2]);
            else
                pareto_pairs_launch<0>(ctx, M, dim3(grid_n.x, splits), g.key, E, n, nullptr, n, nullptr, d_int[1], d_int[2]);
            HIP_TRY(ctx, hipGetLastError());
            pair_tests = (int64_t)n * n;
            if (rank) {
                HIP_TRY(ctx, hipMemcpyAsync(d_int[3], d_int[1], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
                hipLaunchKernelGGL(simplyp::pareto_fill_kernel, grid_n, block, 0, ctx->stream, n, SIMPLYP_PARETO_UNRANKED, d_int[4], (int*)nullptr, (int*)nullptr);
                HIP_TRY(ctx, hipGetLastError());
                simplyp::ParetoPeelArgs p{};
                p.left = d_int[3]; p.rank = d_int[4]; p.front = d_int[5];
                int n_alive = n, side = 0;
                while (n_alive > 0 && (max_fronts == 0 || n_fronts < max_fronts)) {
                    p.n_alive = n_alive; p.front_index = n_fronts; p.alive_out = d_int[6 + side];
                    p.counters = d_head + 4 + 2 * (n_fronts & 1); p.counters_next = d_head + 4 + 2 * ((n_fronts + 1) & 1);
                    hipLaunchKernelGGL(simplyp::pareto_mark_kernel, dim3(blocks(n_alive, T)), block, 0, ctx->stream, p);
                    HIP_TRY(ctx, hipGetLastError());
                    int got[2] = {0, 0};                // the front's size, the members that stay: the one word per front the host reads
                    HIP_TRY(ctx, hipMemcpyAsync(got, p.counters, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    if (got[0] <= 0 || got[0] + got[1] != n_alive)       // a finite strict order always has a front
                        return fail(ctx, SIMPLYP_ERR_DEVICE, "%s: front %d takes %d of %d members and leaves %d", e.me, n_fronts, got[0], n_alive, got[1]);
                    if (n_fronts == 0) n_front0 = got[0];
                    ++n_fronts;
                    if (got[1] > 0 && (max_fronts == 0 || n_fronts < max_fronts)) {
                        const dim3 grid(blocks(got[1], T), blocks(got[0], simplyp::PARETO_JSPLIT));
                        pareto_pairs_launch<2>(ctx, M, grid, g.key, E, got[1], p.alive_out, got[0], p.front, d_int[3], nullptr);
                        HIP_TRY(ctx, hipGetLastError());
                        pair_tests += (int64_t)got[0] * got[1];
                    }
                    p.alive_in = p.alive_out;
                    side ^= 1;
                    n_alive = got[1];
                }
                n_unranked = n_alive;
            }
            hipLaunchKernelGGL(simplyp::pareto_scatter_kernel, grid_n, block, 0, ctx->stream, n, d_int[0], d_int[1], d_int[2], d_int[4],
                               dominated_by, dominates, rank);
        }
        if (int rc = e.end(info ? &info->kernel_ms : nullptr)) return rc;
        if (info) {
            info->pair_tests = pair_tests; info->n_used = n;
            info->n_fronts = n_fronts; info->n_front0 = n_front0; info->n_unranked = n_unranked;
        }
        return SIMPLYP_OK;
    });
}

// ---- the stretch move (simplyp_mcmc.hip.h) ----------------------------------------------------------------------------------
// What the three entries check alike; fills the move.
static int mcmc_move(const Entry& e, int32_t W, int32_t n_dim, int32_t half, double a, uint64_t seed, uint32_t t,
                     simplyp::McmcMove& mv)
{
    if (n_dim < 1 || n_dim > simplyp::MCMC_MAX_DIM)
        return e.refuse("n_dim must be in [1, %d] (got %d)", simplyp::MCMC_MAX_DIM, (int)n_dim);
    if (W < 2 || (W & 1) || W < 2 * n_dim)
        return e.refuse("W must be even and >= 2 n_dim (got W = %d, n_dim = %d)", (int)W, (int)n_dim);
    if (half < 0 || half > 1) return e.refuse("half must be 0 or 1 (got %d)", (int)half);
    if (!(a > 1.0)) return e.refuse("the stretch scale a must be > 1 (got %g)", a);
    mv.W = W; mv.h = W / 2; mv.n_dim = n_dim; mv.half = half; mv.a = a;
    philox_key(seed, mv);
    mv.t = t;
    return SIMPLYP_OK;
}

// What the three entries do alike once their arguments have passed: the cleared info, the four zeroed device counters, the
// start of the timed bracket; and after their launch its end, with the counters read back into the info.
static int mcmc_begin(const Entry& e, simplyp_mcmc_info* info, unsigned*& counters)
{
    if (info) *info = {};
    if (int rc = zeroed_head(e, e.ctx->mcmc, 4 * sizeof(unsigned), 4 * sizeof(unsigned))) return rc;
    counters = (unsigned*)e.ctx->mcmc.ptr;
    return e.begin();
}

static int mcmc_end(const Entry& e, simplyp_mcmc_info* info)
{
    unsigned c[4] = {};
    if (int rc = e.end(info ? &info->kernel_ms : nullptr, c, e.ctx->mcmc.ptr, sizeof(c))) return rc;
    if (info) { info->n_inside = (int32_t)c[0]; info->n_accepted = (int32_t)c[1]; info->n_nan = (int32_t)c[2]; }
    return SIMPLYP_OK;
}

int simplyp_mcmc_propose(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t half, double a, uint64_t seed, uint32_t t,
                         const double* lo, const double* hi, const int32_t* target, const double* theta,
                         double* prop, int32_t* inside, double* member_params, double* f_tdp, simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_mcmc_propose", [&](const Entry& e) -> int {
        simplyp::McmcProposeArgs g{};
        if (int rc = mcmc_move(e, W, n_dim, half, a, seed, t, g.mv)) return rc;
        if (!lo || !hi || !target || !theta || !prop || !inside)
            return e.refuse("lo, hi, target, theta, prop and inside must not be NULL");
        TABLE_TRY(ctx, st::check_box(e.me, n_dim, lo, hi, target, member_params, f_tdp, g.lo, g.hi, g.target, msg));
        g.theta = theta; g.prop = prop; g.inside = inside; g.member_params = member_params; g.f_tdp = f_tdp;
        if (int rc = mcmc_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_mcmc_propose_kernel, dim3(blocks(g.mv.h, simplyp::MCMC_THREADS)),
                           dim3(simplyp::MCMC_THREADS), 0, ctx->stream, g);
        return mcmc_end(e, info);
    });
}

// What the two log-probability entries check alike (`ptrs_ok`, `ptr_names`: the caller's required pointers); fills the
// kernel's arguments but its counters.
static int mcmc_log_prob_args(const Entry& e, int32_t W, int32_t n_dim, int32_t n_out_reaches, bool ptrs_ok, const char* ptr_names,
                              const double* gof, const int32_t* status, const int32_t* inside, const int32_t* pair_var,
                              const int32_t* pair_reach, int32_t n_pairs, const int32_t* m_dim, const double* m_const,
                              const double* prop, double* lp_prop, simplyp::McmcLogProbArgs& g)
{
    simplyp_ctx* const ctx = e.ctx;
    simplyp::McmcMove mv{};
    if (int rc = mcmc_move(e, W, n_dim, 0, 2.0, 0, 0, mv)) return rc;
    if (!ptrs_ok) return e.refuse("%s must not be NULL", ptr_names);
    if (n_out_reaches < 1) return e.refuse("n_out_reaches must be >= 1 (got %d)", (int)n_out_reaches);
    TABLE_TRY(ctx, st::check_pairs(e.me, pair_var, pair_reach, n_pairs, simplyp::MCMC_MAX_PAIRS, n_out_reaches, g.pair_var, g.pair_reach, msg));
    for (int v = 0; v < SIMPLYP_N_GOF_VARS; ++v) {
        if (m_dim[v] < -1 || m_dim[v] >= n_dim)
            return e.refuse("m_dim[%d] = %d is neither -1 nor a row of prop", v, (int)m_dim[v]);
        g.m_dim[v] = m_dim[v]; g.m_const[v] = m_const[v];
    }
    g.h = mv.h; g.R = n_out_reaches; g.n_pairs = n_pairs;
    g.gof = gof; g.status = status; g.inside = inside; g.prop = prop; g.lp_prop = lp_prop;
    return SIMPLYP_OK;
}

int simplyp_mcmc_log_prob(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t n_out_reaches, const double* gof,
                          const int32_t* status, const int32_t* inside, const int32_t* pair_var, const int32_t* pair_reach,
                          int32_t n_pairs, const int32_t* m_dim, const double* m_const, const double* prop, double* lp_prop,
                          simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_mcmc_log_prob", [&](const Entry& e) -> int {
        simplyp::McmcLogProbArgs g{};
        if (int rc = mcmc_log_prob_args(e, W, n_dim, n_out_reaches, gof && pair_var && pair_reach && m_dim && m_const && prop && lp_prop,
                                        "gof, pair_var, pair_reach, m_dim, m_const, prop and lp_prop", gof, status, inside, pair_var,
                                        pair_reach, n_pairs, m_dim, m_const, prop, lp_prop, g))
            return rc;
        if (int rc = mcmc_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_mcmc_log_prob_kernel, dim3(blocks(g.h, simplyp::MCMC_THREADS)),
                           dim3(simplyp::MCMC_THREADS), 0, ctx->stream, g);
        return mcmc_end(e, info);
    });
}

int simplyp_mcmc_log_prob_ar1(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t n_out_reaches, const double* gof,
                              const double* lag, const int32_t* status, const int32_t* inside, const int32_t* pair_var,
                              const int32_t* pair_reach, int32_t n_pairs, const int32_t* m_dim, const double* m_const,
                              const int32_t* phi_dim, const double* phi_const, const double* prop, double* lp_prop,
                              simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_mcmc_log_prob_ar1", [&](const Entry& e) -> int {
        simplyp::McmcLogProbAr1Args a{};
        if (int rc = mcmc_log_prob_args(e, W, n_dim, n_out_reaches,
                                        gof && lag && pair_var && pair_reach && m_dim && m_const && phi_dim && phi_const && prop && lp_prop,
                                        "gof, lag, pair_var, pair_reach, m_dim, m_const, phi_dim, phi_const, prop and lp_prop", gof,
                                        status, inside, pair_var, pair_reach, n_pairs, m_dim, m_const, prop, lp_prop, a.b))
            return rc;
        for (int v = 0; v < SIMPLYP_N_GOF_VARS; ++v) {
            if (phi_dim[v] < -1 || phi_dim[v] >= n_dim)
                return e.refuse("phi_dim[%d] = %d is neither -1 nor a row of prop", v, (int)phi_dim[v]);
            a.phi_dim[v] = phi_dim[v]; a.phi_const[v] = phi_const[v];
        }
        for (int p = 0; p < n_pairs; ++p) {
            const int v = pair_var[p];
            if (phi_dim[v] == -1 && !(phi_const[v] > -1.0 && phi_const[v] < 1.0))
                return e.refuse("phi_const[%d] = %g is not inside (-1, 1)", v, phi_const[v]);
        }
        a.lag = lag;
        if (int rc = mcmc_begin(e, info, a.b.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_mcmc_log_prob_ar1_kernel, dim3(blocks(a.b.h, simplyp::MCMC_THREADS)),
                           dim3(simplyp::MCMC_THREADS), 0, ctx->stream, a);
        return mcmc_end(e, info);
    });
}

int simplyp_mcmc_accept(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t half, double a, uint64_t seed, uint32_t t,
                        const double* prop, const int32_t* inside, const double* lp_prop, double* theta, double* lp,
                        int32_t* n_accept, double* chain_row, simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_mcmc_accept", [&](const Entry& e) -> int {
        simplyp::McmcAcceptArgs g{};
        if (int rc = mcmc_move(e, W, n_dim, half, a, seed, t, g.mv)) return rc;
        if (!prop || !inside || !lp_prop || !theta || !lp || !n_accept)
            return e.refuse("prop, inside, lp_prop, theta, lp and n_accept must not be NULL");
        g.prop = prop; g.inside = inside; g.lp_prop = lp_prop; g.theta = theta; g.lp = lp; g.n_accept = n_accept; g.chain_row = chain_row;
        if (int rc = mcmc_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_mcmc_accept_kernel, dim3(blocks(g.mv.h, simplyp::MCMC_THREADS)),
                           dim3(simplyp::MCMC_THREADS), 0, ctx->stream, g);
        return mcmc_end(e, info);
    });
}

// ---- NSGA-II (include/simplyp_nsga2.h; simplyp_nsga2.h holds the checks and the variation, simplyp_nsga2.hip.h the kernels) ------
namespace sn = simplyp_nsga2;

// What the init and offspring entries fill alike once their own checks have passed: the box, the targets, the key.
static int nsga2_vary_args(const Entry& e, int32_t N, int32_t n_dim, uint64_t seed, uint32_t t, const double* lo, const double* hi,
                           const int32_t* target, double* member_params, double* f_tdp, simplyp::Nsga2VaryArgs& g)
{
    simplyp_ctx* const ctx = e.ctx;
    TABLE_TRY(ctx, st::check_box(e.me, n_dim, lo, hi, target, member_params, f_tdp, g.lo, g.hi, g.target, msg));
    g.N = N; g.n_dim = n_dim; g.t = t;
    philox_key(seed, g);
    g.member_params = member_params; g.f_tdp = f_tdp;
    return SIMPLYP_OK;
}

int simplyp_nsga2_init(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed, const double* lo, const double* hi,
                       const int32_t* target, double* theta, double* member_params, double* f_tdp, simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_nsga2_init", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, sn::check_init(e.me, N, n_dim, theta, msg));
        simplyp::Nsga2VaryArgs g{};
        if (int rc = nsga2_vary_args(e, N, n_dim, seed, 0u, lo, hi, target, member_params, f_tdp, g)) return rc;
        g.child = theta;
        if (int rc = mcmc_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::nsga2_init_kernel, dim3(blocks(N, simplyp::NSGA2_THREADS)), dim3(simplyp::NSGA2_THREADS), 0,
                           ctx->stream, g);
        return mcmc_end(e, info);
    });
}

int simplyp_nsga2_offspring(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed, uint32_t t, int32_t k_c, int32_t k_m,
                            double p_cross, double p_mut, const double* lo, const double* hi, const int32_t* target,
                            const double* theta, const int32_t* rank, const double* crowd, double* child, int32_t* parents,
                            double* member_params, double* f_tdp, simplyp_mcmc_info* info)
{
    return entry(ctx, "simplyp_nsga2_offspring", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, sn::check_offspring(e.me, N, n_dim, k_c, k_m, p_cross, p_mut, theta, rank, crowd, child, msg));
        simplyp::Nsga2VaryArgs g{};
        if (int rc = nsga2_vary_args(e, N, n_dim, seed, t, lo, hi, target, member_params, f_tdp, g)) return rc;
        g.k_c = k_c; g.k_m = k_m; g.p_cross = p_cross; g.p_mut = p_mut;
        g.theta = theta; g.rank = rank; g.crowd = crowd; g.child = child; g.parents = parents;
        if (int rc = mcmc_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::nsga2_offspring_kernel, dim3(blocks(N / 2, simplyp::NSGA2_THREADS)), dim3(simplyp::NSGA2_THREADS), 0,
                           ctx->stream, g);
        return mcmc_end(e, info);
    });
}

int simplyp_nsga2_crowding(simplyp_ctx* ctx, int32_t n, int32_t M, const double* obj, const int32_t* sense, const int32_t* rank,
                           double* crowd, simplyp_pareto_info* info)
{
    return entry(ctx, "simplyp_nsga2_crowding", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, sn::check_crowding(e.me, n, M, obj, sense, rank, crowd, msg));
        if (info) *info = {};
        const size_t plane = (size_t)M * (size_t)n * sizeof(unsigned long long);
        if (int rc = ensure(ctx, ctx->nsga2, 5 * plane)) return rc;
        if (int rc = zeroed_head(e, ctx->mcmc, 4 * sizeof(unsigned), 4 * sizeof(unsigned))) return rc;
        simplyp::Nsga2KeyArgs k{};
        k.n = n; k.M = M; k.obj = obj;
        for (int m = 0; m < M; ++m) k.sense[m] = sense[m];
        k.key = (unsigned long long*)ctx->nsga2.ptr;
        k.run = k.key + (size_t)M * n;
        unsigned* const counters = (unsigned*)ctx->mcmc.ptr;
        const dim3 block(simplyp::NSGA2_THREADS), grid_n(blocks(n, simplyp::NSGA2_THREADS));
        const dim3 grid_pairs(grid_n.x, blocks(n, simplyp::NSGA2_JSPLIT));
        if (int rc = e.begin()) return rc;
        hipLaunchKernelGGL(simplyp::nsga2_keys_kernel, grid_n, block, 0, ctx->stream, k);
        HIP_TRY(ctx, hipGetLastError());
#define NSGA2_CASE(MP)                                                                                                      \
    hipLaunchKernelGGL((simplyp::nsga2_crowd_pairs_kernel<MP>), grid_pairs, block, 0, ctx->stream, k.key, (int)M, (int)n, rank, k.run)
        switch (M) {                                    // M padded to the next compiled size
        case 1: NSGA2_CASE(1); break;
        case 2: NSGA2_CASE(2); break;
        case 3: NSGA2_CASE(3); break;
        case 4: NSGA2_CASE(4); break;
        case 5: case 6: NSGA2_CASE(6); break;
        default: NSGA2_CASE(8); break;
        }
#undef NSGA2_CASE
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::nsga2_crowd_finish_kernel, grid_n, block, 0, ctx->stream, (int)n, (int)M, rank, k.run, crowd, counters);
        unsigned c[4] = {};
        if (int rc = e.end(info ? &info->kernel_ms : nullptr, c, counters, sizeof(c))) return rc;
        if (info) { info->pair_tests = (int64_t)n * n; info->n_used = (int32_t)c[0]; }
        return SIMPLYP_OK;
    });
}

int simplyp_nsga2_select(simplyp_ctx* ctx, int32_t n, int32_t N, const int32_t* rank, const double* crowd, int32_t* position,
                         int32_t* survivor, int32_t n_rows, const double* rows_in, double* rows_out, int32_t* rank_out,
                         double* crowd_out, simplyp_pareto_info* info)
{
    return entry(ctx, "simplyp_nsga2_select", [&](const Entry& e) -> int {
        TABLE_TRY(ctx, sn::check_select(e.me, n, N, rank, crowd, position, survivor, n_rows, rows_in, rows_out, msg));
        if (info) *info = {};
        simplyp::Nsga2GatherArgs g{};
        g.n = n; g.N = N; g.n_rows = n_rows; g.position = position; g.rank = rank; g.crowd = crowd; g.rows_in = rows_in;
        g.survivor = survivor; g.rank_out = rank_out; g.crowd_out = crowd_out; g.rows_out = rows_out;
        const dim3 block(simplyp::NSGA2_THREADS), grid_n(blocks(n, simplyp::NSGA2_THREADS));
        if (int rc = e.begin()) return rc;
        HIP_TRY(ctx, hipMemsetAsync(position, 0, (size_t)n * sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(simplyp::nsga2_position_kernel, dim3(grid_n.x, blocks(n, simplyp::NSGA2_JSPLIT)), block, 0, ctx->stream,
                           (int)n, rank, crowd, position);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(simplyp::nsga2_gather_kernel, grid_n, block, 0, ctx->stream, g);
        if (int rc = e.end(info ? &info->kernel_ms : nullptr)) return rc;
        if (info) { info->pair_tests = (int64_t)n * n; info->n_used = N; }
        return SIMPLYP_OK;
    });
}

// ---- multi-start Nelder-Mead (simplyp_neldermead.hip.h) ---------------------------------------------------------------------
// What the two entries check alike.
static int nm_shape(const Entry& e, int32_t S, int32_t n_dim)
{
    if (n_dim < 1 || n_dim > simplyp::MCMC_MAX_DIM)
        return e.refuse("n_dim must be in [1, %d] (got %d)", simplyp::MCMC_MAX_DIM, (int)n_dim);
    if (S < 1 || S > (1 << 28)) return e.refuse("S must be in [1, 2^28] (got %d)", (int)S);
    return SIMPLYP_OK;
}

// As mcmc_begin and mcmc_end, with the eight counters of the simplexes.
static int nm_begin(const Entry& e, simplyp_nm_info* info, unsigned*& counters)
{
    if (info) *info = {};
    if (int rc = zeroed_head(e, e.ctx->nm, 8 * sizeof(unsigned), 8 * sizeof(unsigned))) return rc;
    counters = (unsigned*)e.ctx->nm.ptr;
    return e.begin();
}

static int nm_end(const Entry& e, simplyp_nm_info* info)
{
    unsigned c[8] = {};
    if (int rc = e.end(info ? &info->kernel_ms : nullptr, c, e.ctx->nm.ptr, sizeof(c))) return rc;
    if (info) {
        info->n_active = (int32_t)c[0]; info->n_converged = (int32_t)c[1]; info->n_shrinking = (int32_t)c[2];
        info->n_nonfinite_start = (int32_t)c[3]; info->n_inside = (int32_t)c[4];
    }
    return SIMPLYP_OK;
}

int simplyp_nm_propose(simplyp_ctx* ctx, int32_t S, int32_t n_dim, const double* lo, const double* hi, const int32_t* target,
                       const double* sim, const int32_t* istate, double* prop, int32_t* inside, double* member_params,
                       double* f_tdp, simplyp_nm_info* info)
{
    return entry(ctx, "simplyp_nm_propose", [&](const Entry& e) -> int {
        if (int rc = nm_shape(e, S, n_dim)) return rc;
        if (!lo || !hi || !target || !sim || !istate || !prop || !inside)
            return e.refuse("lo, hi, target, sim, istate, prop and inside must not be NULL");
        simplyp::NmProposeArgs g{};
        TABLE_TRY(ctx, st::check_box(e.me, n_dim, lo, hi, target, member_params, f_tdp, g.lo, g.hi, g.target, msg));
        g.S = S; g.n_dim = n_dim;
        g.sim = sim; g.istate = istate; g.prop = prop; g.inside = inside; g.member_params = member_params; g.f_tdp = f_tdp;
        if (int rc = nm_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_nm_propose_kernel, dim3(blocks(S, simplyp::NM_THREADS)),
                           dim3(simplyp::NM_THREADS), 0, ctx->stream, g);
        return nm_end(e, info);
    });
}

int simplyp_nm_update(simplyp_ctx* ctx, int32_t S, int32_t n_dim, int32_t max_iter, double xatol, double fatol,
                      const double* prop, const int32_t* inside, const double* lp_prop, double* sim, double* fsim,
                      int32_t* istate, double* history, int32_t history_rows, simplyp_nm_info* info)
{
    return entry(ctx, "simplyp_nm_update", [&](const Entry& e) -> int {
        if (int rc = nm_shape(e, S, n_dim)) return rc;
        if (max_iter < 1) return e.refuse("max_iter must be >= 1 (got %d)", (int)max_iter);
        if (!(xatol >= 0.0) || !(fatol >= 0.0))
            return e.refuse("xatol and fatol must be >= 0 (got %g, %g)", xatol, fatol);
        if (history_rows < 0) return e.refuse("history_rows must be >= 0 (got %d)", (int)history_rows);
        if (!prop || !inside || !lp_prop || !sim || !fsim || !istate)
            return e.refuse("prop, inside, lp_prop, sim, fsim and istate must not be NULL");
        simplyp::NmUpdateArgs g{};
        g.S = S; g.n_dim = n_dim; g.max_iter = max_iter; g.history_rows = history ? history_rows : 0; g.xatol = xatol; g.fatol = fatol;
        g.prop = prop; g.inside = inside; g.lp_prop = lp_prop; g.sim = sim; g.fsim = fsim; g.istate = istate; g.history = history;
        if (int rc = ensure(ctx, ctx->nm_work, (size_t)(n_dim + 1) * (size_t)(n_dim + 1) * (size_t)S * sizeof(double))) return rc;
        g.work = (double*)ctx->nm_work.ptr;
        if (int rc = nm_begin(e, info, g.counters)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_nm_update_kernel, dim3(blocks(S, simplyp::NM_THREADS)),
                           dim3(simplyp::NM_THREADS), 0, ctx->stream, g);
        return nm_end(e, info);
    });
}

// ---- Sobol' indices (simplyp_sobol.hip.h) -----------------------------------------------------------------------------------
// What the two entries check alike.
static int sobol_shape(const Entry& e, int32_t N, int32_t n_dim)
{
    if (N < simplyp::SOBOL_MIN_N || N > simplyp::SOBOL_MAX_N)
        return e.refuse("N must be in [%d, %d] (got %d)", simplyp::SOBOL_MIN_N, simplyp::SOBOL_MAX_N, (int)N);
    if (n_dim < 1 || n_dim > simplyp::SOBOL_MAX_DIM)
        return e.refuse("n_dim must be in [1, %d] (got %d)", simplyp::SOBOL_MAX_DIM, (int)n_dim);
    return SIMPLYP_OK;
}

int simplyp_sobol_design(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed, const double* lo, const double* hi,
                         const int32_t* target, const double* unit, double* x, double* member_params, double* f_tdp,
                         simplyp_sobol_info* info)
{
    return entry(ctx, "simplyp_sobol_design", [&](const Entry& e) -> int {
        if (int rc = sobol_shape(e, N, n_dim)) return rc;
        if (!lo || !hi || !target || !x) return e.refuse("lo, hi, target and x must not be NULL");
        simplyp::SobolDesignArgs g{};
        TABLE_TRY(ctx, st::check_box(e.me, n_dim, lo, hi, target, member_params, f_tdp, g.lo, g.hi, g.target, msg));
        g.N = N; g.n_dim = n_dim; philox_key(seed, g);
        g.unit = unit; g.x = x; g.member_params = member_params; g.f_tdp = f_tdp;
        if (info) *info = {};
        if (int rc = e.begin()) return rc;
        const int E = N * (n_dim + 2);
        hipLaunchKernelGGL(simplyp::simplyp_sobol_design_kernel, dim3(blocks(E, simplyp::SOBOL_THREADS)),
                           dim3(simplyp::SOBOL_THREADS), 0, ctx->stream, g);
        return e.end(info ? &info->kernel_ms : nullptr);
    });
}

int simplyp_sobol_indices(simplyp_ctx* ctx, int32_t N, int32_t n_dim, int32_t n_rows, const double* table, const int32_t* status,
                          int32_t n_boot, uint64_t seed, double* sums, int32_t* n_used, double* indices, simplyp_sobol_info* info)
{
    return entry(ctx, "simplyp_sobol_indices", [&](const Entry& e) -> int {
        if (int rc = sobol_shape(e, N, n_dim)) return rc;
        if (n_rows < 0) return e.refuse("n_rows must be >= 0 (got %d)", (int)n_rows);
        if (n_boot < 0 || n_boot > simplyp::SOBOL_MAX_BOOT)
            return e.refuse("n_boot must be in [0, %d] (got %d)", simplyp::SOBOL_MAX_BOOT, (int)n_boot);
        if (info) { *info = {}; info->n_resamples = 1 + n_boot; }
        if (n_rows == 0) return SIMPLYP_OK;
        if (!table || !indices) return e.refuse("table and indices must not be NULL");
        const int B = 1 + n_boot, T = 2 * n_dim + 2, tiles = (T + 15) / 16;
        if ((long long)n_rows * B > (1LL << 31) - 1 - simplyp::SOBOL_THREADS)
            return e.refuse("n_rows (1 + n_boot) must stay below 2^31 (got %d rows, %d resamples)", (int)n_rows, B);
        const int Npad = (N + simplyp::SOBOL_KC - 1) / simplyp::SOBOL_KC * simplyp::SOBOL_KC;
        auto up = [](size_t b) { return (b + 255) / 256 * 256; };
        const size_t o_valid = 256, o_mu = o_valid + up((size_t)Npad), o_used = o_mu + up((size_t)n_rows * sizeof(double));
        const size_t o_counts = o_used + up((size_t)B * sizeof(int32_t));
        const size_t o_sums = o_counts + up((size_t)B * Npad * sizeof(uint16_t));
        const size_t total = o_sums + (sums ? 0 : up((size_t)B * n_rows * T * sizeof(double)));
        if (int rc = ensure(ctx, ctx->sobol, total)) return rc;
        char* base = (char*)ctx->sobol.ptr;
        simplyp::SobolArgs g{};
        g.N = N; g.Npad = Npad; g.n_dim = n_dim; g.n_rows = n_rows; g.B = B;
        philox_key(seed, g);
        g.table = table; g.status = status;
        g.n_valid = (int32_t*)base; g.valid = (uint8_t*)(base + o_valid); g.mu = (double*)(base + o_mu);
        g.n_used = n_used ? n_used : (int32_t*)(base + o_used);
        g.counts = (uint16_t*)(base + o_counts);
        g.sums = sums ? sums : (double*)(base + o_sums);
        g.indices = indices;
        const hipEvent_t ev_contract = ctx->ev_lap[0];
        const dim3 threads(simplyp::SOBOL_THREADS);
        if (int rc = e.begin()) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_sobol_mean_kernel, dim3((unsigned)n_rows), threads, 0, ctx->stream, g);
        const size_t lds = std::max<size_t>((size_t)Npad * sizeof(uint16_t), simplyp::SOBOL_THREADS * sizeof(uint32_t));
        hipLaunchKernelGGL(simplyp::simplyp_sobol_counts_kernel, dim3((unsigned)B), threads, lds, ctx->stream, g);
        HIP_TRY(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
        const dim3 grid((unsigned)n_rows, blocks(B, simplyp::SOBOL_RB));
        if (tiles == 1) hipLaunchKernelGGL(simplyp::simplyp_sobol_contract_kernel<1>, grid, threads, 0, ctx->stream, g);
        else if (tiles == 2) hipLaunchKernelGGL(simplyp::simplyp_sobol_contract_kernel<2>, grid, threads, 0, ctx->stream, g);
        else hipLaunchKernelGGL(simplyp::simplyp_sobol_contract_kernel<3>, grid, threads, 0, ctx->stream, g);
        HIP_TRY(ctx, hipEventRecord(ev_contract, ctx->stream));
        const long long cells = (long long)n_rows * B;
        hipLaunchKernelGGL(simplyp::simplyp_sobol_epilogue_kernel, dim3(blocks(cells, simplyp::SOBOL_THREADS)),
                           threads, 0, ctx->stream, g);
        int32_t n_valid = 0;
        if (int rc = e.end(info ? &info->kernel_ms : nullptr, &n_valid, g.n_valid, sizeof(n_valid))) return rc;
        if (info) {
            float f = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&f, ctx->ev_start, ctx->ev_main));
            info->counts_ms = f;
            HIP_TRY(ctx, hipEventElapsedTime(&f, ctx->ev_main, ev_contract));
            info->contract_ms = f;
            info->flops = 2LL * B * n_rows * N * T;
            info->bytes_workspace = (int64_t)total;
            info->n_valid = n_valid;
        }
        return SIMPLYP_OK;
    });
}

// ---- the particle filter's steps (simplyp_particle.hip.h) ---------------------------------------------------------------------
constexpr size_t PF_HEAD_BYTES = 256;      // the PfResult at the head of ctx->pf

// What the five entries do alike once their arguments have passed: the workspace (`work_bytes` behind the result slot), the
// zeroed result, the start of the timed bracket.  Nothing is launched before this.
static int pf_open(const Entry& e, simplyp_pf_info* info, size_t work_bytes, simplyp::PfResult*& res, char*& work)
{
    if (info) *info = {};
    if (int rc = zeroed_head(e, e.ctx->pf, PF_HEAD_BYTES + work_bytes, sizeof(simplyp::PfResult))) return rc;
    res = (simplyp::PfResult*)e.ctx->pf.ptr;
    work = (char*)e.ctx->pf.ptr + PF_HEAD_BYTES;
    return e.begin();
}

// After the entry's launches: the end of the bracket, with the result read back into the info.
static int pf_close(const Entry& e, simplyp_pf_info* info)
{
    simplyp::PfResult r{};
    if (int rc = e.end(info ? &info->kernel_ms : nullptr, &r, e.ctx->pf.ptr, sizeof(r))) return rc;
    if (info) {
        info->lw_max = r.lw_max; info->sum_w = r.sum_w; info->sum_w2 = r.sum_w2; info->T = r.T;
        info->n_alive = (int32_t)r.n_alive; info->n_nan = (int32_t)r.n_nan; info->n_unique = (int32_t)r.n_unique;
        info->n_bad = (int32_t)r.n_bad; info->n_outside = (int32_t)r.n_outside;
    }
    return SIMPLYP_OK;
}

static int pf_shape(const Entry& e, int64_t E)
{
    if (E < 1 || E > simplyp_resample::MAX_E)
        return e.refuse("E must be in [1, 2^%d] (got %lld)", simplyp_resample::MAX_LOG2_E, (long long)E);
    return SIMPLYP_OK;
}

int simplyp_pf_loglik(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask, const int32_t* out_reaches,
                      int32_t n_out_reaches, const double* out, const int32_t* member_of_slot, const double* f_tdp,
                      const double* reach_params, const double* obs, const int32_t* pair_var, const int32_t* pair_reach,
                      int32_t n_pairs, const double* err_m, const int32_t* status, double* lw, double* inc, int32_t accumulate,
                      simplyp_pf_info* info)
{
    return entry(ctx, "simplyp_pf_loglik", [&](const Entry& e) -> int {
        TableView t;
        const bool ptrs_ok = out && f_tdp && reach_params && obs && pair_var && pair_reach && err_m && lw;
        if (int rc = check_table(e, dims, out_mask, out_reaches, n_out_reaches, ptrs_ok, false, t)) return rc;
        if (int rc = pf_shape(e, t.E)) return rc;
        const int E = t.E, S = t.S, D = t.D, R = t.R;
        simplyp::PfLoglikArgs g{};
        TABLE_TRY(ctx, st::check_pairs(e.me, pair_var, pair_reach, n_pairs, simplyp::PF_MAX_PAIRS, R, g.pair_var, g.pair_reach, msg));
        // the observation days of every pair in the window, ascending, and what was observed: shared by all particles
        Staging up;
        up.put(t.reach_of);
        const size_t o_day = up.ints.size();
        for (int p = 0; p < n_pairs; ++p) {
            const double* ob = obs + ((size_t)pair_reach[p] * SIMPLYP_N_GOF_VARS + pair_var[p]) * D;
            for (int d = 0; d < D; ++d)
                if (ob[d] == ob[d]) { up.ints.push_back(d); up.dbl.push_back(ob[d]); }
            g.day_ptr[p + 1] = (int)up.dbl.size();
        }
        char* work = nullptr;
        if (int rc = pf_open(e, info, up.bytes(), g.res, work)) return rc;
        if (int rc = up.upload(e, work)) return rc;
        g.E = E; g.R = R; g.n_pairs = n_pairs; g.accumulate = accumulate != 0;
        g.out = out; g.col_stride = (long long)D * R * E;
        std::copy(t.col, t.col + 4, g.col);
        g.reach_of = up.d_ints; g.day = up.d_ints + o_day; g.obs = up.d_dbl;
        g.member_of_slot = member_of_slot; g.f_tdp = f_tdp;
        g.a_catch = reach_params + (size_t)SIMPLYP_PR_A_CATCH * S * E;
        g.err_m = err_m; g.status = status; g.lw = lw; g.inc = inc;
        hipLaunchKernelGGL(simplyp::simplyp_pf_loglik_kernel, dim3(blocks(E, simplyp::PF_THREADS)), dim3(simplyp::PF_THREADS), 0, ctx->stream, g);
        return pf_close(e, info);          // synchronises: the host lists outlive their copies
    });
}

int simplyp_pf_weights(simplyp_ctx* ctx, int32_t E, const double* lw, double* w, uint64_t* q, simplyp_pf_info* info)
{
    return entry(ctx, "simplyp_pf_weights", [&](const Entry& e) -> int {
        if (int rc = pf_shape(e, E)) return rc;
        if (!lw || !w || !q) return e.refuse("lw, w and q must not be NULL");
        simplyp::PfWeightsArgs g{};
        g.E = E; g.n_blocks = (int)blocks(E, simplyp::PF_THREADS);
        g.lw = lw; g.w = w; g.q = (unsigned long long*)q;
        char* work = nullptr;
        if (int rc = pf_open(e, info, (size_t)3 * g.n_blocks * sizeof(double), g.res, work)) return rc;
        g.part_max = (double*)work; g.part_sum = (double*)work + g.n_blocks;
        const dim3 grid((unsigned)g.n_blocks), one(1), threads(simplyp::PF_THREADS);
        hipLaunchKernelGGL(simplyp::simplyp_pf_max_kernel, grid, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_max_finish_kernel, one, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_weights_kernel, grid, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_sum_finish_kernel, one, threads, 0, ctx->stream, g);
        return pf_close(e, info);
    });
}

int simplyp_pf_resample(simplyp_ctx* ctx, int32_t E, const uint64_t* q, uint64_t seed, uint32_t t, int32_t* ancestors,
                        int32_t* offspring, simplyp_pf_info* info)
{
    return entry(ctx, "simplyp_pf_resample", [&](const Entry& e) -> int {
        if (int rc = pf_shape(e, E)) return rc;
        if (!q || !ancestors) return e.refuse("q and ancestors must not be NULL");
        simplyp::PfResampleArgs g{};
        g.E = E; g.n_blocks = (int)blocks(E, simplyp::PF_THREADS);
        g.q = (const unsigned long long*)q; g.ancestors = ancestors; g.offspring = offspring;
        philox_key(seed, g); g.t = t;
        char* work = nullptr;
        if (int rc = pf_open(e, info, ((size_t)E + g.n_blocks) * sizeof(uint64_t), g.res, work)) return rc;
        g.C = (unsigned long long*)work; g.block_sum = g.C + E;
        if (offspring) HIP_TRY(ctx, hipMemsetAsync(offspring, 0, (size_t)E * sizeof(int32_t), ctx->stream));
        const dim3 grid((unsigned)g.n_blocks), one(1), threads(simplyp::PF_THREADS);
        hipLaunchKernelGGL(simplyp::simplyp_pf_scan_block_kernel, grid, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_scan_sums_kernel, one, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_scan_add_kernel, grid, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_search_kernel, grid, threads, 0, ctx->stream, g);
        hipLaunchKernelGGL(simplyp::simplyp_pf_offspring_kernel, grid, threads, 0, ctx->stream, g);
        return pf_close(e, info);
    });
}

int simplyp_gather_members(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const int32_t* ancestors, const void* src, void* dst,
                           simplyp_pf_info* info)
{
    return entry(ctx, "simplyp_gather_members", [&](const Entry& e) -> int {
        if (int rc = pf_shape(e, E)) return rc;
        if (n_rows < 0 || n_rows > (int64_t)0x7FFFFFFF)
            return e.refuse("n_rows must be in [0, 2^31) (got %lld)", (long long)n_rows);
        if (info) *info = {};                           // here, not only in pf_open: no rows is a success, and the refusals below come after it
        if (n_rows == 0) return SIMPLYP_OK;
        if (!ancestors || !src || !dst) return e.refuse("ancestors, src and dst must not be NULL");
        const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)n_rows * (uintptr_t)E * 8u;
        if (a < b + bytes && b < a + bytes) return e.refuse("src and dst overlap (the gather is out of place)");
        simplyp::PfGatherArgs g{};
        g.E = E; g.n_rows = n_rows; g.ancestors = ancestors;
        g.src = (const unsigned long long*)src; g.dst = (unsigned long long*)dst;
        char* work = nullptr;
        if (int rc = pf_open(e, info, 0, g.res, work)) return rc;
        const long long row_blocks = (n_rows + simplyp::PF_GATHER_ROWS - 1) / simplyp::PF_GATHER_ROWS;
        hipLaunchKernelGGL(simplyp::simplyp_gather_members_kernel, dim3(blocks(E, simplyp::PF_THREADS), (unsigned)std::min<long long>(row_blocks, 65535)),
                           dim3(simplyp::PF_THREADS), 0, ctx->stream, g);
        return pf_close(e, info);
    });
}

int simplyp_pf_jitter(simplyp_ctx* ctx, int32_t E, int32_t n_dim, uint64_t seed, uint32_t t, double a, const double* centre,
                      const double* scale, const double* lo, const double* hi, const int32_t* target, double* theta,
                      double* member_params, double* f_tdp, simplyp_pf_info* info)
{
    return entry(ctx, "simplyp_pf_jitter", [&](const Entry& e) -> int {
        if (int rc = pf_shape(e, E)) return rc;
        if (n_dim < 1 || n_dim > simplyp::PF_MAX_DIM)
            return e.refuse("n_dim must be in [1, %d] (got %d)", simplyp::PF_MAX_DIM, (int)n_dim);
        if (!centre || !scale || !lo || !hi || !target || !theta)
            return e.refuse("centre, scale, lo, hi, target and theta must not be NULL");
        if (!std::isfinite(a)) return e.refuse("a must be finite (got %g)", a);
        simplyp::PfJitterArgs g{};
        TABLE_TRY(ctx, st::check_box(e.me, n_dim, lo, hi, target, member_params, f_tdp, g.lo, g.hi, g.target, msg));
        for (int d = 0; d < n_dim; ++d) {
            if (!std::isfinite(centre[d]) || !(scale[d] >= 0.0) || !std::isfinite(scale[d]))
                return e.refuse("centre[%d] must be finite and scale[%d] finite and >= 0 (got %g, %g)", d, d, centre[d], scale[d]);
            g.centre[d] = centre[d]; g.scale[d] = scale[d];
        }
        g.E = E; g.n_dim = n_dim; g.a = a; g.t = t;
        philox_key(seed, g);
        g.theta = theta; g.member_params = member_params; g.f_tdp = f_tdp;
        char* work = nullptr;
        if (int rc = pf_open(e, info, 0, g.res, work)) return rc;
        hipLaunchKernelGGL(simplyp::simplyp_pf_jitter_kernel, dim3(blocks(E, simplyp::PF_THREADS)), dim3(simplyp::PF_THREADS), 0, ctx->stream, g);
        return pf_close(e, info);
    });
}

void* simplyp_host_alloc(int64_t bytes)
{
    void* p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void simplyp_host_free(void* p) { if (p) (void)hipHostFree(p); }

void* simplyp_device_alloc(simplyp_ctx* ctx, int64_t bytes)
{
    if (!ctx || bytes <= 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&p, (size_t)bytes) != hipSuccess) {
        fail(ctx, SIMPLYP_ERR_NOMEM, "hipMalloc(%lld bytes) failed", (long long)bytes);
        return nullptr;
    }
    return p;
}

void simplyp_device_free(simplyp_ctx* ctx, void* p)
{
    if (!ctx || !p) return;
    (void)hipSetDevice(ctx->device);
    (void)hipFree(p);
}

int simplyp_memcpy_h2d(simplyp_ctx* ctx, void* dst, const void* src, int64_t bytes)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SIMPLYP_OK;
}

int simplyp_memcpy_d2h(simplyp_ctx* ctx, void* dst, const void* src, int64_t bytes)
{
    if (!ctx) return SIMPLYP_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SIMPLYP_OK;
}

int simplyp_eval_units(simplyp_ctx* ctx, int32_t which, int32_t n, const double* in, double* out)
{
    return entry(ctx, "simplyp_eval_units", [&](const Entry& e) -> int {
        if (which < 0 || which > 7 || n < 0 || (n > 0 && (!in || !out))) return e.refuse("bad arguments");
        if (n == 0) return SIMPLYP_OK;
        if (which == 6)             // the right-hand sides: four lanes per row
            hipLaunchKernelGGL(simplyp::eval_rhs_kernel, dim3(blocks(n, 16)), dim3(64), 0, ctx->stream, (int)n, in, out);
        else if (which == 7)        // the step-rule pieces
            hipLaunchKernelGGL(simplyp::eval_step_kernel, dim3(blocks(n, 64)), dim3(64), 0, ctx->stream, (int)n, in, out);
        else
            hipLaunchKernelGGL(simplyp::eval_units_kernel, dim3(blocks(n, 64)), dim3(64), 0, ctx->stream, (int)which, (int)n, in, out);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return SIMPLYP_OK;
    });
}

int simplyp_order_members(simplyp_ctx* ctx, int32_t E, const uint32_t* cost, int32_t where, int32_t* perm, double* diag, uint64_t* keys)
{
    return entry(ctx, "simplyp_order_members", [&](const Entry& e) -> int {
        namespace sp = simplyp;
        if (E < 1) return e.refuse("E must be >= 1 (got %d)", (int)E);
        if (!cost || !perm) return e.refuse("cost and perm must not be NULL");
        if (where != 0 && where != 1) return e.refuse("where must be 0 (the device's kernels) or 1 (the host rule) (got %d)", (int)where);
        if (where == 0 && E > sp::ORD_MAX_E)
            return e.refuse("the device orders at most %d members (got %d); where = 1 orders any number", sp::ORD_MAX_E, (int)E);
        if (where == 1 && keys) return e.refuse("keys are the device's sorted total-cost keys: where = 1 has none");
        if (where == 1) {
            std::vector<uint32_t> h_cost((size_t)sp::ORD_WIN * E);
            HIP_TRY(ctx, hipMemcpyAsync(h_cost.data(), cost, h_cost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            std::vector<int32_t> h_perm;
            double h_diag[simplyp_order::DIAG_DOUBLES];
            order_members(h_cost, sp::ORD_WIN, E, h_perm, diag ? h_diag : nullptr);
            HIP_TRY(ctx, hipMemcpyAsync(perm, h_perm.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            if (diag) HIP_TRY(ctx, hipMemcpyAsync(diag, h_diag, sizeof(h_diag), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return SIMPLYP_OK;
        }
        if (int rc = ensure(ctx, ctx->order, order_workspace_bytes(E))) return rc;
        if (int rc = order_members_device(ctx, cost, perm, ctx->order.ptr, E)) return rc;
        // where order_members_device has put its arrays in the workspace (its layout, restated: tests/test_gpu_order_direct.py
        // compares what is read here with the costs' own moments, covariance and sorted keys)
        const int P = order_sort_keys(E), n_groups = (E + sp::ORD_THREADS - 1) / sp::ORD_THREADS;
        const unsigned long long* key = (const unsigned long long*)(((uintptr_t)ctx->order.ptr + 7) & ~(uintptr_t)7);
        const double* part_cov = (const double*)(key + P) + (size_t)n_groups * 2 * sp::ORD_WIN;
        const double* moments = part_cov + (size_t)n_groups * sp::ORD_NCOV;
        if (diag) {
            hipLaunchKernelGGL(sp::order_diag_kernel, dim3(1), dim3(64), 0, ctx->stream, E, n_groups, part_cov, moments,
                               (const float*)(moments + 2 * sp::ORD_WIN), diag);
            if (int rc = e.launched()) return rc;
        }
        if (keys) HIP_TRY(ctx, hipMemcpyAsync(keys, key, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return SIMPLYP_OK;
    });
}

}  // extern "C"
