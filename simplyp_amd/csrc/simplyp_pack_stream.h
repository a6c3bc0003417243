// simplyp_pack_stream.h -- host side of the packed output stream: a pinned staging ring, the copies of packed records into
// it, a dispatcher thread that waits for each landed record, and a pool of decode threads that turn it into fp64 rows of the
// caller's table (simplyp_pack.h is the codec).  Shared by the library (simplyp_hip.hip) and tools/pack_gate.hip.
//
// Order of events for record number k (records are numbered in the order submit() is called):
//   submit      waits until record k - n_slots has been released, enqueues the record's copy (first row, directory and the body
//               as far as its cursor went are contiguous) and an event behind it on the caller's stream;
//   dispatcher  hipEventSynchronize on that event -- its own event, nobody else waits on it -- then marks k landed;
//   workers     every worker decodes ITS member range (whole 64-member blocks) of every record, in order; the last one to
//               finish record k releases the slot.  Records are therefore released in order.  A column predicted from another
//               one is decoded after that one's record of the same chunk: the worker reads its own rows of it back from the
//               destination table.
//   finish      no more records: returns when the dispatcher and every worker have run out of work and are joined.
#pragma once

#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "simplyp_pack.h"

namespace simplyp_pack {

// Decode threads: what this process may run on -- the affinity mask, capped by OMP_NUM_THREADS where that is set -- minus two,
// for the caller and the copier.  Never the machine's core count.  SIMPLYP_DECODE_THREADS overrides.
inline int decode_threads()
{
    if (const char* env = getenv("SIMPLYP_DECODE_THREADS")) {
        const int v = atoi(env);
        if (v >= 1) return v > 64 ? 64 : v;
    }
    int n = 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (const char* omp = getenv("OMP_NUM_THREADS")) {
        const int v = atoi(omp);
        if (v >= 1 && v < n) n = v;
    }
    n -= 2;
    return n < 1 ? 1 : (n > 32 ? 32 : n);
}

// The CPUs of the NUMA node the GPU hangs off, among those the calling thread may run on (sysfs; false when there is no such
// entry, one node only, or nothing left).  The staging ring lives on that node (ROCr places pinned memory there), and so does
// a destination table allocated by a thread bound there: a decode thread on another socket reads and writes across the
// inter-socket link -- measured on C3's shapes: 693 ... 1383 ms per pass with the pool unbound, 720.5 +- 1 bound.
inline bool gpu_node_cpus(int device, cpu_set_t* out, int* node_out = nullptr)
{
    char bdf[64] = {0}, path[256];
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) return false;
    for (char* c = bdf; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    int node = -1;
    FILE* f = fopen(path, "r");
    if (!f || fscanf(f, "%d", &node) != 1) node = -1;
    if (f) fclose(f);
    if (node < 0) return false;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return false;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    CPU_ZERO(out);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) { fclose(f); return false; }
    int lo = 0, hi = 0, n = 0;
    while (fscanf(f, "%d", &lo) == 1) {
        hi = lo;
        int ch = fgetc(f);
        if (ch == '-') { if (fscanf(f, "%d", &hi) != 1) hi = lo; ch = fgetc(f); }
        for (int c = lo; c <= hi && c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &allowed)) { CPU_SET(c, out); ++n; }
        if (ch != ',') break;
    }
    fclose(f);
    if (node_out) *node_out = node;
    return n > 0;
}

// Best effort: restrict the calling thread to those CPUs.  Returns the node, or -1 when nothing was changed.
inline int bind_thread_to_gpu_node(int device)
{
    cpu_set_t set;
    int node = -1;
    if (!gpu_node_cpus(device, &set, &node) || sched_setaffinity(0, sizeof(set), &set) != 0) return -1;
    return node;
}

struct PackJob {
    const unsigned char* dev_rec = nullptr;   // the record in device memory
    Layout L;
    int nd = 0;
    size_t copy_bytes = 0;                    // what travels: simplyp_pack::copy_bytes(L, the record's word cursor)
    double* dst = nullptr;                    // the column's first row of the chunk in the caller's table
    const double* xdst = nullptr;             // the predictor column's, in the same table (nullptr: previous day)
    size_t stride = 0;                        // doubles per row of that table
    int slot = 0;
};

struct Tally {
    int n_packed = 0, n_raw = 0;              // records routed packed / raw
    unsigned n_overflow = 0;                  // overflow blocks of the packed ones
    size_t link_bytes = 0;                    // what the packed ones put on the link
    int raw_of_col[32] = {};                  // records routed raw, per column
    int raw_why[4] = {};                      // n_raw by reason, indexed by Route ([PACKED] stays 0)
    size_t raw_bytes = 0;                     // what the raw ones put on the link
};

// Packed or raw, for every record of chunk `c` in column order -- the one place that decides it.  counters(j, overflow_blocks,
// words) hands over record (c, j)'s two counters.  A record travels raw when its own counters and the size of its rows say so
// (route_of), and when the column it is predicted from travels raw in this chunk: its decoder reads that column's rows from the
// host table, where a raw copy lands in no order with the decode pool.  Per column either packed(job) -- the record at
// `dev_recs` (null: the caller keeps the record itself) to the columns of the table at `host` -- or raw(offset in doubles,
// bytes) of that table.
template <class Counters, class Packed, class Raw>
void route_chunk(const Table& t, int c, const unsigned char* dev_recs, double* host, Tally& tally, Counters&& counters, Packed&& packed,
                 Raw&& raw)
{
    const Layout L = t.layout_of(c);
    bool is_raw[32] = {};
    for (int j = 0; j < t.n_cols; ++j) {
        unsigned overflow_blocks = 0;
        size_t words = 0;
        counters(j, overflow_blocks, words);
        const int k = t.pred[j];
        Route why = route_of(L, overflow_blocks, words, t.cap, t.raw_bytes(c));
        if (why == PACKED && k >= 0 && is_raw[k]) why = RAW_FOLLOWS;
        is_raw[j] = why != PACKED;
        if (is_raw[j]) {
            ++tally.n_raw; ++tally.raw_of_col[j]; ++tally.raw_why[why]; tally.raw_bytes += t.raw_bytes(c);
            raw(t.offset(j, c), t.raw_bytes(c));
            continue;
        }
        PackJob job;
        job.dev_rec = dev_recs ? dev_recs + t.record(c, j) * t.stride : nullptr;
        job.L = L;
        job.nd = t.days(c);
        job.copy_bytes = copy_bytes(L, words);
        job.dst = host + t.offset(j, c);
        job.xdst = k >= 0 ? host + t.offset(k, c) : nullptr;
        job.stride = (size_t)t.E;
        ++tally.n_packed; tally.n_overflow += overflow_blocks; tally.link_bytes += job.copy_bytes;
        packed(job);
    }
}

class PackStream {
public:
    static constexpr size_t RING_MAX = (size_t)1 << 30;
    ~PackStream() { release(); }

    // Grow-only ring of pinned slots of `slot_bytes` each (as many as fit 1 GiB, at most `max_jobs`, at least 2) and a job
    // table for `max_jobs` records; starts the dispatcher and `n_threads` decode workers (0: records are released as they land,
    // nothing is decoded -- the gate's "decode off").  Called by the thread that will wait for the run.
    hipError_t start(int device, size_t E, size_t slot_bytes, int max_jobs, int n_threads)
    {
        finish();
        if (spin_ != events_spin_) {
            for (hipEvent_t ev : events_) (void)hipEventDestroy(ev);
            events_.clear();
            events_spin_ = spin_;
        }
        slot_bytes = round_up(slot_bytes, 4096);
        int want = (int)(RING_MAX / slot_bytes);
        if (want > max_jobs) want = max_jobs;
        if (want < 2) want = 2;
        const size_t bytes = (size_t)want * slot_bytes;
        if (bytes > ring_bytes_) {
            if (ring_) { (void)hipHostFree(ring_); ring_ = nullptr; ring_bytes_ = 0; }
            hipError_t err = hipHostMalloc((void**)&ring_, bytes, hipHostMallocDefault);
            if (err != hipSuccess) return err;
            ring_bytes_ = bytes;
        }
        while ((int)events_.size() < want) {
            hipEvent_t ev;
            hipError_t err = hipEventCreateWithFlags(&ev, hipEventDisableTiming | (spin_ ? 0u : hipEventBlockingSync));
            if (err != hipSuccess) return err;
            events_.push_back(ev);
        }
        device_ = device; E_ = E; slot_bytes_ = slot_bytes; n_slots_ = want; T_ = n_threads;
        jobs_.assign((size_t)max_jobs, PackJob());
        remaining_.reset(new std::atomic<int>[(size_t)max_jobs]);
        n_issued_ = n_landed_ = n_released_ = 0; total_ = -1; error_ = 0;
        busy_s_.assign((size_t)(T_ > 0 ? T_ : 1), 0.0);
        running_ = true;
        dispatcher_ = std::thread([this] { dispatch_main(); });
        for (int t = 0; t < T_; ++t) workers_.emplace_back([this, t] { worker_main(t); });
        return hipSuccess;
    }

    // Enqueue record `j` on `stream` (called by one thread, the copier).  Blocks while the ring is full.
    hipError_t submit(PackJob j, hipStream_t stream)
    {
        int seq;
        {
            std::unique_lock<std::mutex> lk(m_);
            seq = n_issued_;
            if (seq >= (int)jobs_.size()) return hipErrorInvalidValue;
            cv_.wait(lk, [&] { return seq - n_released_ < n_slots_; });
        }
        j.slot = seq % n_slots_;
        unsigned char* to = ring_ + (size_t)j.slot * slot_bytes_;
        // one plain copy: the body follows the first row and the directory directly
        hipError_t err = hipMemcpyAsync(to, j.dev_rec, j.copy_bytes, hipMemcpyDeviceToHost, stream);
        hipError_t err2 = hipEventRecord(events_[(size_t)j.slot], stream);      // recorded whatever happened: the dispatcher waits on it
        if (err == hipSuccess) err = err2;
        if (err != hipSuccess && !error_) error_ = (int)err;
        packed_bytes_ += j.copy_bytes;
        jobs_[(size_t)seq] = j;
        remaining_[(size_t)seq].store(T_, std::memory_order_relaxed);
        { std::lock_guard<std::mutex> lk(m_); n_issued_ = seq + 1; }
        cv_.notify_all();
        return err;
    }

    // No more records.  Returns once every submitted record is decoded and released and the threads are joined; idempotent.
    void finish()
    {
        if (!running_) return;
        { std::lock_guard<std::mutex> lk(m_); total_ = n_issued_; }
        cv_.notify_all();
        if (dispatcher_.joinable()) dispatcher_.join();
        for (std::thread& w : workers_) if (w.joinable()) w.join();
        workers_.clear();
        running_ = false;
    }

    // The dispatcher's wait for a landed record: blocking (the default: it leaves its CPU to the decode pool) or spinning.
    void set_spin(bool spin) { spin_ = spin; }
    int error() const { return error_; }
    int n_slots() const { return n_slots_; }
    size_t take_packed_bytes() { const size_t b = packed_bytes_; packed_bytes_ = 0; return b; }
    double busy_seconds_mean() const { double s = 0; for (double b : busy_s_) s += b; return s / (double)busy_s_.size(); }

    void release()
    {
        finish();
        for (hipEvent_t ev : events_) (void)hipEventDestroy(ev);
        events_.clear();
        if (ring_) { (void)hipHostFree(ring_); ring_ = nullptr; ring_bytes_ = 0; }
    }

private:
    void dispatch_main()
    {
        (void)hipSetDevice(device_);
        for (int seq = 0;; ++seq) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return n_issued_ > seq || total_ >= 0; });
                if (n_issued_ <= seq) return;
            }
            hipError_t err = hipEventSynchronize(events_[(size_t)jobs_[(size_t)seq].slot]);
            if (err != hipSuccess && !error_) error_ = (int)err;
            {
                std::lock_guard<std::mutex> lk(m_);
                n_landed_ = seq + 1;
                if (T_ == 0) n_released_ = seq + 1;
            }
            cv_.notify_all();
        }
    }

    void worker_main(int t)
    {
        (void)bind_thread_to_gpu_node(device_);      // this thread only; the caller's own placement is the caller's business
        FpDefault fp;                                // the ratio predictor rounds as the device does, whatever the caller had set
        (void)fp;
        // member ranges are whole blocks
        const size_t G = (E_ + GROUP - 1) / GROUP;
        const size_t e0 = G * (size_t)t / (size_t)T_ * GROUP;
        const size_t e1 = std::min(E_, G * (size_t)(t + 1) / (size_t)T_ * GROUP);
        for (int seq = 0;; ++seq) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return n_landed_ > seq || (total_ >= 0 && seq >= total_); });
                if (n_landed_ <= seq) return;
            }
            const PackJob& j = jobs_[(size_t)seq];
            const unsigned char* rec = ring_ + (size_t)j.slot * slot_bytes_;
            const auto t0 = std::chrono::steady_clock::now();
            if (e1 > e0 && !error_) decode_range(rec, j.L, j.nd, E_, e0, e1, j.dst, j.xdst, j.stride);
            __builtin_ia32_sfence();      // the non-temporal stores are globally visible before the range counts as done
            busy_s_[(size_t)t] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (remaining_[(size_t)seq].fetch_sub(1, std::memory_order_acq_rel) == 1) {
                { std::lock_guard<std::mutex> lk(m_); n_released_ = seq + 1; }
                cv_.notify_all();
            }
        }
    }

    unsigned char* ring_ = nullptr;
    size_t ring_bytes_ = 0, slot_bytes_ = 0, E_ = 0, packed_bytes_ = 0;
    std::vector<hipEvent_t> events_;
    std::vector<PackJob> jobs_;
    std::unique_ptr<std::atomic<int>[]> remaining_;
    std::vector<double> busy_s_;
    std::mutex m_;
    std::condition_variable cv_;
    int n_issued_ = 0, n_landed_ = 0, n_released_ = 0, total_ = -1;     // guarded by m_
    std::atomic<int> error_{0};
    int device_ = 0, n_slots_ = 0, T_ = 0;
    bool running_ = false, spin_ = false, events_spin_ = false;
    std::thread dispatcher_;
    std::vector<std::thread> workers_;
};

}  // namespace simplyp_pack
