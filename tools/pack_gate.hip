// pack_gate.hip -- go / no-go for the packed output stream, without a model run: the real shapes (one pinned destination of
// the whole table, the pinned staging ring, a device buffer of packed records -- random bits under a valid directory whose row
// widths are each column's mean on the model's table (51, 51, 52, 52 bits, and 35 for the last column,
// which is decoded against the third with the second-order ratio predictor: its spans carry the ORDER2 flag) --, the real schedule
// (two copy streams taken in turn, one record per chunk-column, the library's router, dispatcher and decode pool from
// simplyp_pack_stream.h), against the raw copies of the same table in the same session.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I simplyp_amd/csrc -o pack_gate tools/pack_gate.hip -lpthread
//   ./pack_gate [E=100000] [D=10957] [n_cols=5] [chunk_days=64] [repeats=3]      (PACK_GATE_NO_BIND=1: leave the main thread unbound)
//
// Prints a markdown table: per mode the wall time, the link rate (bytes that crossed / time until the last copy had landed),
// the decode rate (table bytes / mean busy time of a decode thread) -- for the raw copies, for packed copies with decode off,
// and for T = 8, 12, 14 decode threads and the T the library would pick.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "simplyp_pack_stream.h"

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        hipError_t e__ = (call);                                                                             \
        if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__)); return 1; }     \
    } while (0)

__global__ void fill_kernel(unsigned long long* p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long x = i * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        p[i] = x;
    }
}

// A valid directory for every block of every record: one span, every row `w` bits wide, blocks in order; the span of a column
// that has a predictor column is flagged second order.
__global__ void directory_kernel(unsigned char* dev, simplyp_pack::Table t, int G, const int* width_of_col)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)t.n_chunks() * t.n_cols * G) return;
    const int rec = (int)(i / G), g = (int)(i % G), w = width_of_col[rec % t.n_cols];
    const simplyp_pack::Layout L = t.layout_of(rec / t.n_cols);
    unsigned char* dir = dev + (size_t)rec * t.stride + L.off_dir + (size_t)g * L.dir_stride;
    *(uint32_t*)dir = (uint32_t)((size_t)g * L.rows * w);
    for (int r = 0; r < L.rows; ++r) dir[L.off_widths + r] = (unsigned char)w;
    if (L.rows > 0 && t.pred[rec % t.n_cols] >= 0) dir[L.off_widths] |= simplyp_pack::ORDER2;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv)
{
    using namespace simplyp_pack;
    const size_t E = argc > 1 ? (size_t)atol(argv[1]) : 100000;
    const size_t D = argc > 2 ? (size_t)atol(argv[2]) : 10957;
    const int n_cols = argc > 3 ? atoi(argv[3]) : 5;
    const int chunk = argc > 4 ? atoi(argv[4]) : 64;
    const int repeats = argc > 5 ? atoi(argv[5]) : 3;
    // PP (the fifth column) against Msus (the third)
    int32_t pred[32];
    for (int j = 0; j < 32; ++j) pred[j] = j == 4 ? 2 : -1;
    if (n_cols < 1 || n_cols > 32) { fprintf(stderr, "1 .. 32 columns\n"); return 1; }
    const Table t = make_table(n_cols, (int)D, (int)E, chunk, pred);
    const int G = (int)((E + GROUP - 1) / GROUP), n_chunks = t.n_chunks(), n_rec = n_chunks * n_cols;
    const size_t table_bytes = (size_t)n_cols * D * E * sizeof(double);
    size_t dev_bytes = (size_t)n_rec * t.stride;
    if (dev_bytes < table_bytes) dev_bytes = table_bytes;
    printf("shape: %zu members x %zu days x %d columns, %d-day chunks: %d records of %.1f MB (overflow capacity %u blocks), table %.2f GB\n",
           E, D, n_cols, chunk, n_rec, t.stride / 1e6, t.cap, table_bytes / 1e9);

    unsigned char* dev = nullptr;
    double* host = nullptr;
    CHECK(hipSetDevice(0));
    // bench.py binds its thread to the GPU's NUMA node before it allocates the table (engine.bind_host_thread_to_gpu_numa_node);
    // the decode pool binds itself there in any case
    if (!getenv("PACK_GATE_NO_BIND")) printf("main thread bound to the GPU's NUMA node: %d (-1 = not bound)\n", simplyp_pack::bind_thread_to_gpu_node(0));
    CHECK(hipMalloc((void**)&dev, dev_bytes));
    hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, (unsigned long long*)dev, dev_bytes / 8);
    const int widths[5] = {51, 51, 52, 52, 35};
    std::vector<int> width_of_col((size_t)n_cols);
    for (int j = 0; j < n_cols; ++j) width_of_col[(size_t)j] = widths[j % 5];
    int* dev_widths = nullptr;
    CHECK(hipMalloc((void**)&dev_widths, (size_t)n_cols * sizeof(int)));
    CHECK(hipMemcpy(dev_widths, width_of_col.data(), (size_t)n_cols * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(directory_kernel, dim3((unsigned)(((size_t)n_rec * G + 255) / 256)), dim3(256), 0, 0, dev, t, G, dev_widths);
    CHECK(hipDeviceSynchronize());
    double t0 = now_s();
    CHECK(hipHostMalloc((void**)&host, table_bytes, hipHostMallocDefault));
    printf("pinned destination allocated in %.1f s\n", now_s() - t0);
    hipStream_t streams[2];
    for (hipStream_t& s : streams) CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    printf("\n| mode | run | wall ms | link GB/s | bytes on the link GB | decode GB/s per pool |\n|---|---|---|---|---|---|\n");
    // raw: what the library does today -- one plain copy per chunk-column, straight into the destination
    for (int r = 0; r < repeats; ++r) {
        t0 = now_s();
        unsigned n = 0;
        for (int c = 0; c < n_chunks; ++c)
            for (int j = 0; j < n_cols; ++j)
                CHECK(hipMemcpyAsync(host + t.offset(j, c), (const double*)dev + t.offset(j, c), t.raw_bytes(c), hipMemcpyDeviceToHost, streams[n++ % 2]));
        for (hipStream_t s : streams) CHECK(hipStreamSynchronize(s));
        const double dt = now_s() - t0;
        printf("| raw fp64 | %d | %.1f | %.2f | %.2f | - |\n", r, dt * 1e3, table_bytes / dt / 1e9, table_bytes / 1e9);
        fflush(stdout);
    }
    PackStream ps;
    const int t_auto = decode_threads();
    // decode off twice: the dispatcher waiting on blocking events, then on spinning ones; the rest with blocking events
    const int modes[] = {0, 0, 8, 12, 14, t_auto};
    for (int mi = 0; mi < 6; ++mi) {
        const int T = modes[mi];
        ps.set_spin(mi == 1);
        for (int r = 0; r < repeats; ++r) {
            CHECK(ps.start(0, E, t.stride, n_rec, T));
            ps.take_packed_bytes();
            t0 = now_s();
            unsigned n = 0;
            Tally tally;
            hipError_t err = hipSuccess;
            // the library's router on synthetic counters: no overflow blocks, a cursor that is the column's width in every row
            for (int c = 0; c < n_chunks; ++c)
                route_chunk(t, c, dev, host, tally,
                            [&](int j, unsigned& overflow_blocks, size_t& words) {
                                overflow_blocks = 0; words = (size_t)G * (size_t)(t.days(c) - 1) * (size_t)width_of_col[(size_t)j];
                            },
                            [&](const PackJob& job) { if (err == hipSuccess) err = ps.submit(job, streams[n++ % 2]); },
                            [&](size_t, size_t) { if (err == hipSuccess) err = hipErrorInvalidValue; });     // (no width passes the capacity)
            CHECK(err);
            for (hipStream_t s : streams) CHECK(hipStreamSynchronize(s));
            const double t_link = now_s() - t0;
            ps.finish();
            const double dt = now_s() - t0;
            const size_t sent = ps.take_packed_bytes();
            if (ps.error()) { fprintf(stderr, "copy error %d\n", ps.error()); return 1; }
            char dec[32] = "-";
            if (T > 0) snprintf(dec, sizeof(dec), "%.1f", table_bytes / ps.busy_seconds_mean() / 1e9);
            printf("| packed, %s%d decode threads%s (%d ring slots) | %d | %.1f | %.2f | %.2f | %s |\n", mi == 5 ? "auto = " : "",
                   T, mi == 1 ? ", spinning dispatcher" : "", ps.n_slots(), r, dt * 1e3, sent / t_link / 1e9, sent / 1e9, dec);
            fflush(stdout);
        }
    }
    ps.release();
    (void)hipHostFree(host);
    (void)hipFree(dev);
    (void)hipFree(dev_widths);
    return 0;
}
