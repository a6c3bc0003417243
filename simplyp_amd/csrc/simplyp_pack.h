// simplyp_pack.h -- the lossless codec of the packed output stream: one definition, compiled for the device (the pack
// epilogue of the task-queue kernel, simplyp_fetch_packed) and for the host (the decode pool, the plain C++ encoder of the
// CPU test).  Values travel as their 64-bit patterns.
//
// Per (column, member): z = zigzag(u[d] - p[d]) modulo 2^64, where u[d] is the day's pattern and p[d] its prediction:
//   pred_col = -1   p[d] = u[d-1], the previous day of the same column;
//   pred_col =  k   X = column k of the same chunk, Y = this column, r1 = Y[d-1] / X[d-1], r2 = the r1 of the row before (the
//                   same fp64 value, carried along the chunk, not recomputed).  Per 64-member block and span of 64 delta rows
//                   the encoder chooses (predict2())
//                     first order    p[d] = pattern of X[d] * r1, or
//                     second order   p[d] = pattern of X[d] * ((r1 + r1) - r2): the ratio extrapolated one day,
//                   whichever makes the span smaller (first order on a tie, and where second order alone would make the block
//                   an overflow block).  Division, multiplication, doubling and subtraction are separate IEEE operations,
//                   correctly rounded on both sides of the link.  A second-order pattern that is +-0 or has an all-ones
//                   exponent is replaced by the first-order pattern, and such a first-order pattern by u[d-1].  The first delta
//                   row of a chunk has no r2 and is first order in any span.
// All members see the same weather, so the 64 members of a block have small z on the same days and large z on the same days:
// every row of a block (64 members, one day) is stored at the bit width of its widest z.
//
// One record per (time chunk, column), contiguous so that it is one plain copy:
//   row 0      [E] fp64          the chunk's first day, raw: chunks decode independently of each other
//   directory  [G] entries       per 64-member block: [n_spans] uint32 -- where each span of 64 delta rows starts in the body,
//                                in 8-byte words -- then one width byte (0 .. 64) per delta row (entry padded to 4 bytes);
//                                bit 7 (ORDER2) of a span's first width byte: the span is coded second order
//   body                         per span its rows one after the other; a row of width w is the 64 z at w bits each, value i at
//                                bit i * w: 8 * w bytes.  Spans take their place with one atomic add on the record's word
//                                cursor, so their order is whatever the run made it.  8 bytes of padding follow the last row.
// Two counters per record live outside it (one array per run, zeroed with one memset): [0] blocks that hold any z >= 2^56
// ("overflow blocks"), [1] the word cursor.  A record travels raw -- the copier then sends that chunk-column from the fp64
// table -- when its body passes its fixed capacity, or when it has more than overflow_capacity() overflow blocks and its
// packed copy would not be smaller than its rows (route_of()).  The count of overflow blocks alone sends nothing raw: it is a
// reported statistic, and it sizes the record's capacity.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#if defined(__HIPCC__)
#define SIMPLYP_PACK_HD __host__ __device__
#else
#define SIMPLYP_PACK_HD
#endif

namespace simplyp_pack {

constexpr int GROUP = 64;        // members per block = lanes of a wavefront
constexpr int SPAN = 64;         // delta rows whose widths one wavefront holds, one per lane
constexpr int Z_BITS = 56;       // a block with a wider z counts as an overflow block; the host's fast path ends here too

SIMPLYP_PACK_HD inline uint64_t zigzag(uint64_t delta) { return (delta << 1) ^ (uint64_t)((int64_t)delta >> 63); }
SIMPLYP_PACK_HD inline uint64_t unzigzag(uint64_t z) { return (z >> 1) ^ (0ull - (z & 1ull)); }
SIMPLYP_PACK_HD inline uint64_t encode(uint64_t u, uint64_t pred) { return zigzag(u - pred); }
SIMPLYP_PACK_HD inline uint64_t decode(uint64_t z, uint64_t pred) { return pred + unzigzag(z); }
SIMPLYP_PACK_HD inline bool fits(uint64_t z) { return (z >> Z_BITS) == 0ull; }
SIMPLYP_PACK_HD inline int width_of(uint64_t z) { return z ? 64 - __builtin_clzll(z) : 0; }

// The ratio predictor.  The only floating-point operations of the codec: IEEE division and multiplication, round to nearest,
// denormals kept (the host side runs under FpDefault).  Whether the result is used is decided on its pattern.
SIMPLYP_PACK_HD inline uint64_t predict(uint64_t x, uint64_t x_prev, uint64_t y_prev)
{
    const double p = __builtin_bit_cast(double, x) * (__builtin_bit_cast(double, y_prev) / __builtin_bit_cast(double, x_prev));
    const uint64_t pb = __builtin_bit_cast(uint64_t, p), mag = pb & 0x7FFFFFFFFFFFFFFFull;
    return (mag == 0ull || (mag >> 52) == 0x7FFull) ? y_prev : pb;
}

constexpr unsigned char ORDER2 = 0x80;        // in a span's first width byte: the span is coded second order

// Both orders of the ratio predictor.  r1 = Y[d-1] / X[d-1] comes back for the next row, whose r_prev it is; p1 is predict()'s
// pattern, p2 that of X[d] * (2 r1 - r_prev) with p1 in its place where it is unusable.  One division as before; the doubling
// is exact (or inf, and then the product is unusable).
SIMPLYP_PACK_HD inline void predict2(uint64_t x, uint64_t x_prev, uint64_t y_prev, double r_prev, double& r1, uint64_t& p1, uint64_t& p2)
{
    const double xd = __builtin_bit_cast(double, x);
    r1 = __builtin_bit_cast(double, y_prev) / __builtin_bit_cast(double, x_prev);
    const uint64_t b1 = __builtin_bit_cast(uint64_t, xd * r1), m1 = b1 & 0x7FFFFFFFFFFFFFFFull;
    p1 = (m1 == 0ull || (m1 >> 52) == 0x7FFull) ? y_prev : b1;
    const double twice = r1 + r1;
    const double slope = twice - r_prev;
    const uint64_t b2 = __builtin_bit_cast(uint64_t, xd * slope), m2 = b2 & 0x7FFFFFFFFFFFFFFFull;
    p2 = (m2 == 0ull || (m2 >> 52) == 0x7FFull) ? p1 : b2;
}

// Overflow blocks a record's capacity allows for: an eighth of its n_groups blocks (the model's flux columns need 2.3 %), and
// three more for a small ensemble -- each counted as wholly raw fp64 in Layout::body_cap_words, which fixes the record stride,
// the ring slots and the pack buffer.  That is what a block with a z >= 2^56 cost when it was stored whole and raw; now it
// merely has some wide rows, so a record may hold more such blocks than this and still fit and travel packed: beyond this
// count route_of() goes by the size of the packed copy.
SIMPLYP_PACK_HD inline unsigned overflow_capacity(int n_groups) { return (unsigned)n_groups / 8u + 3u; }

struct Layout {
    size_t off_dir, dir_stride, off_widths;   // directory: bytes from the start of the record, bytes per entry, widths inside an entry
    size_t off_body;
    size_t body_cap_words;                    // what the body may hold: 7 bytes per value and `cap` blocks of raw fp64
    size_t bytes;                             // whole record at capacity, padding included (a multiple of 256)
    int rows, n_spans;                        // delta rows, spans of them
};

SIMPLYP_PACK_HD inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

SIMPLYP_PACK_HD inline Layout layout(size_t E, int nd, unsigned cap)
{
    Layout L;
    const size_t G = (E + GROUP - 1) / GROUP;
    L.rows = nd - 1;
    L.n_spans = (L.rows + SPAN - 1) / SPAN;
    L.off_dir = round_up(E * sizeof(double), 256);
    L.off_widths = (size_t)L.n_spans * sizeof(uint32_t);
    L.dir_stride = round_up(L.off_widths + (size_t)L.rows, 4);
    L.off_body = round_up(L.off_dir + G * L.dir_stride, 256);
    L.body_cap_words = ((size_t)L.rows * E * 7 + 7) / 8 + (size_t)cap * (size_t)nd * GROUP;
    L.bytes = round_up(L.off_body + L.body_cap_words * 8 + 8, 256);
    return L;
}

// What crosses the link for a record whose cursor stands at `words`.
SIMPLYP_PACK_HD inline size_t copy_bytes(const Layout& L, size_t words) { return L.off_body + words * 8 + 8; }

// Why a record travels raw (Tally counts them apart).  RAW_FOLLOWS is the router's: the column is predicted from a raw one.
enum Route { PACKED = 0, RAW_PAST_CAPACITY = 1, RAW_NOT_SMALLER = 2, RAW_FOLLOWS = 3 };

// Packed or raw by the record's own counters; `raw_bytes` is what its rows would put on the link (Table::raw_bytes).
//   past the capacity   the device skipped the spans beyond it, so the record is incomplete;
//   not smaller         more overflow blocks than `cap` AND a packed copy at least as large as the rows.  Many overflow blocks
//                       alone decide nothing: such a block has some wide rows, and the record usually stays well below its rows.
//                       The size alone decides nothing either: a small ragged record (200 members in 256 lanes) would go raw
//                       for its padding.
SIMPLYP_PACK_HD inline Route route_of(const Layout& L, unsigned overflow_blocks, size_t words, unsigned cap, size_t raw_bytes)
{
    if (words > L.body_cap_words) return RAW_PAST_CAPACITY;
    if (overflow_blocks > cap && copy_bytes(L, words) >= raw_bytes) return RAW_NOT_SMALLER;
    return PACKED;
}

// A [n_cols][rows][E] fp64 table cut into chunks of `chunk_days` rows (the last one may be shorter), and its records: record
// (c, j) is chunk c of column j, records lie `stride` bytes apart in chunk-major order.
struct Table {
    int n_cols, rows, chunk_days, E;
    unsigned cap;                             // overflow blocks a record may hold
    size_t stride;                            // bytes between records: a full chunk's record at capacity
    int pred[32];                             // per column: the EARLIER column it is predicted from, or -1 (previous day)

    SIMPLYP_PACK_HD int n_chunks() const { return (rows + chunk_days - 1) / chunk_days; }
    SIMPLYP_PACK_HD int first_day(int c) const { return c * chunk_days; }
    SIMPLYP_PACK_HD int days(int c) const { return rows - first_day(c) < chunk_days ? rows - first_day(c) : chunk_days; }
    SIMPLYP_PACK_HD size_t record(int c, int j) const { return (size_t)c * (size_t)n_cols + (size_t)j; }
    SIMPLYP_PACK_HD size_t offset(int j, int c) const { return ((size_t)j * (size_t)rows + (size_t)first_day(c)) * (size_t)E; }   // doubles
    SIMPLYP_PACK_HD size_t raw_bytes(int c) const { return (size_t)days(c) * (size_t)E * sizeof(double); }    // a column's rows of chunk c
    SIMPLYP_PACK_HD Layout layout_of(int c) const { return layout((size_t)E, days(c), cap); }
};

// Records travel in column order and a decode thread needs its rows of the predictor column in the host table first: pred_col
// (may be NULL = all -1) holds -1 or a column before j, for at most 32 columns.
SIMPLYP_PACK_HD inline bool pred_cols_ok(const int32_t* pred_col, int n_cols)
{
    for (int j = 0; pred_col && j < n_cols; ++j)
        if (pred_col[j] < -1 || pred_col[j] >= j) return false;
    return n_cols <= 32;
}

SIMPLYP_PACK_HD inline Table make_table(int n_cols, int rows, int E, int chunk_days, const int32_t* pred_col)
{
    Table t;
    t.n_cols = n_cols; t.rows = rows; t.chunk_days = chunk_days; t.E = E;
    t.cap = overflow_capacity((E + GROUP - 1) / GROUP);
    t.stride = layout((size_t)E, chunk_days, t.cap).bytes;
    for (int j = 0; j < 32; ++j) t.pred[j] = (pred_col && j < n_cols) ? pred_col[j] : -1;
    return t;
}

#if defined(__HIPCC__)
constexpr int BATCH = 8;                        // rows a wavefront handles together
constexpr int LDS_WORDS = BATCH * GROUP;        // LDS a packing wavefront needs: one row image per row of a batch

// v[i]: this lane's value of row i of a batch.  Returns, in every lane, the maximum over all lanes of row (lane & 7): three
// exchange steps in which a lane gives away the half of the rows its partner keeps, then three plain steps -- 10 shuffles for 8
// rows, 6 deep, where 8 separate reductions take 48.
__device__ __forceinline__ int wave_max_rows(const int (&v)[BATCH], int lane)
{
    const bool b2 = (lane & 4) != 0, b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
    int a[4], b[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = max(b2 ? v[j + 4] : v[j], __shfl_xor(b2 ? v[j] : v[j + 4], 4));
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = max(b1 ? a[j + 2] : a[j], __shfl_xor(b1 ? a[j] : a[j + 2], 2));
    int c = max(b0 ? b[1] : b[0], __shfl_xor(b0 ? b[0] : b[1], 1));
    for (int m = 8; m < GROUP; m <<= 1) c = max(c, __shfl_xor(c, m));
    return c;
}

// LDS operations of one wavefront execute in order; this keeps the compiler to the order they are written in.
__device__ __forceinline__ void lds_order()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// One wavefront packs its own block: members g*64 .. g*64+63 of `nd` rows of one column.  `rows` points at the column's first
// row of the chunk, `xrows` at the predictor column's (nullptr: previous day), `stride` is doubles per row.  `count` are the
// record's two counters, `lds` LDS_WORDS words of LDS that belong to this wavefront alone.
// Per span of 64 delta rows: a first pass finds the widths (lane r keeps row r's, a lane prefix sum gives the row offsets), one
// atomic add takes the span's place in the body, a second pass reads the rows again (L2) and packs them -- each lane ORs its z
// into the row's LDS image, which then leaves as w coalesced 8-byte stores.  Both passes take the rows eight at a time, so
// that a batch costs one round of loads, shuffles and LDS operations, not eight.
__device__ __forceinline__ void pack_block(const double* rows, const double* xrows, size_t stride, int nd, int E, int g, int lane,
                                           unsigned char* rec, const Layout& L, unsigned* count, unsigned long long* lds)
{
    const int e = g * GROUP + lane;
    const bool live = e < E;
    const unsigned long long* src = (const unsigned long long*)rows + (live ? e : 0);
    const unsigned long long* xsrc = xrows ? (const unsigned long long*)xrows + (live ? e : 0) : src;
    const bool ratio = xrows != nullptr;                       // wave-uniform
    if (live) ((unsigned long long*)rec)[e] = src[0];
    unsigned char* dir = rec + L.off_dir + (size_t)g * L.dir_stride;
    unsigned long long* body = (unsigned long long*)(rec + L.off_body);
    unsigned long long big = 0ull;
    double rprev = 0.0;                                        // r1 of the row before (ratio columns), carried over the spans
    for (int s = 0; s < L.n_spans; ++s) {
        const int d_first = 1 + s * SPAN, n = min(SPAN, nd - d_first);      // rows d_first .. d_first + n - 1
        unsigned long long prev = live ? src[(size_t)(d_first - 1) * stride] : 0ull;
        unsigned long long xprev = (live && ratio) ? xsrc[(size_t)(d_first - 1) * stride] : 0ull;
        const unsigned long long prev0 = prev, xprev0 = xprev;
        const double rprev0 = rprev;
        unsigned long long big1 = 0ull, big2 = 0ull;           // this span's, under either order
        int wmine = 0, wmine2 = 0;
        for (int k0 = 0; k0 < n; k0 += BATCH) {
            unsigned long long u[BATCH], x[BATCH];
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {
                const bool in = live && k0 + i < n;
                u[i] = in ? src[(size_t)(d_first + k0 + i) * stride] : 0ull;
                x[i] = (in && ratio) ? xsrc[(size_t)(d_first + k0 + i) * stride] : 0ull;
            }
            int wv[BATCH];
            if (ratio) {
                int wv2[BATCH];
#pragma unroll
                for (int i = 0; i < BATCH; ++i) {
                    const bool in = live && k0 + i < n;
                    double r1;
                    uint64_t p1, p2;
                    predict2(x[i], xprev, prev, rprev, r1, p1, p2);
                    if (d_first + k0 + i == 1) p2 = p1;        // the chunk's first delta row
                    const unsigned long long z1 = in ? encode(u[i], p1) : 0ull, z2 = in ? encode(u[i], p2) : 0ull;
                    prev = u[i]; xprev = x[i]; rprev = r1;
                    big1 |= z1 >> Z_BITS; big2 |= z2 >> Z_BITS;
                    wv[i] = width_of(z1); wv2[i] = width_of(z2);
                }
                const int w2 = wave_max_rows(wv2, lane);
                if ((lane & ~(BATCH - 1)) == k0) wmine2 = w2;
            } else {
#pragma unroll
                for (int i = 0; i < BATCH; ++i) {
                    const bool in = live && k0 + i < n;
                    const unsigned long long z = in ? encode(u[i], prev) : 0ull;
                    prev = u[i];
                    big1 |= z >> Z_BITS;
                    wv[i] = width_of(z);
                }
            }
            const int w = wave_max_rows(wv, lane);             // of row k0 + (lane & 7)
            if ((lane & ~(BATCH - 1)) == k0) wmine = w;
        }
        const double rend = rprev;
        // second order where it makes the span smaller and does not make an overflow block of a clean one (wave-uniform)
        bool order2 = false;
        if (ratio) {
            int t1 = wmine, t2 = wmine2;
            for (int m = 1; m < GROUP; m <<= 1) { t1 += __shfl_xor(t1, m); t2 += __shfl_xor(t2, m); }
            order2 = t2 < t1 && !(__ballot(big2 != 0ull) != 0ull && __ballot(big1 != 0ull) == 0ull);
        }
        if (order2) wmine = wmine2;
        big |= order2 ? big2 : big1;
        int inc = wmine;                                       // inclusive lane prefix sum of the widths = words
        for (int o = 1; o < GROUP; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        const int excl = inc - wmine;
        const unsigned total = (unsigned)__builtin_amdgcn_readlane(inc, GROUP - 1);
        unsigned base = 0u;
        if (total != 0u) {
            if (lane == 0) base = atomicAdd(count + 1, total);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        }
        if ((size_t)base + total > L.body_cap_words) continue; // (wave-uniform) past the capacity: the record travels raw
        if (lane == 0) ((uint32_t*)dir)[s] = base;
        if (lane < n) dir[L.off_widths + (size_t)(d_first - 1 + lane)] = (unsigned char)(wmine | ((order2 && lane == 0) ? ORDER2 : 0));
        if (total == 0u) continue;
        prev = prev0; xprev = xprev0; rprev = rprev0;
        for (int k0 = 0; k0 < n; k0 += BATCH) {
            unsigned long long u[BATCH], x[BATCH];
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {
                const bool in = live && k0 + i < n;
                u[i] = in ? src[(size_t)(d_first + k0 + i) * stride] : 0ull;
                x[i] = (in && ratio) ? xsrc[(size_t)(d_first + k0 + i) * stride] : 0ull;
            }
#pragma unroll
            for (int i = 0; i < BATCH; ++i) __hip_atomic_store(&lds[i * GROUP + lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            lds_order();
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {
                const bool in = live && k0 + i < n;
                unsigned long long p = prev;
                if (order2) {
                    double r1;
                    uint64_t p1, p2;
                    predict2(x[i], xprev, prev, rprev, r1, p1, p2);
                    p = d_first + k0 + i == 1 ? p1 : p2;
                    rprev = r1;
                } else if (ratio) {
                    p = predict(x[i], xprev, prev);
                }
                const unsigned long long z = in ? encode(u[i], p) : 0ull;
                prev = u[i]; xprev = x[i];
                const int w = __builtin_amdgcn_readlane(wmine, k0 + i);       // (0 beyond the span's last row)
                const int bit = lane * w, wi = bit >> 6, sh = bit & 63;
                if (z != 0ull) {
                    __hip_atomic_fetch_or(&lds[i * GROUP + wi], z << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (sh + w > 64) __hip_atomic_fetch_or(&lds[i * GROUP + wi + 1], z >> (64 - sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            lds_order();
#pragma unroll
            for (int i = 0; i < BATCH; ++i) {
                const int w = __builtin_amdgcn_readlane(wmine, k0 + i);
                const int off = __builtin_amdgcn_readlane(excl, k0 + i);
                if (lane < w)
                    body[(size_t)base + (size_t)off + (size_t)lane] = __hip_atomic_load(&lds[i * GROUP + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            lds_order();
        }
        rprev = rend;
    }
    if (__ballot(big != 0ull) != 0ull && lane == 0) atomicAdd(count, 1u);
}

// What a packing kernel knows of a run's records (Table's device half); `buf` null = the run does not pack.
struct PackArgs {
    unsigned char* buf = nullptr;             // [n_chunks][cols] records, `stride` bytes apart
    unsigned* count = nullptr;                // [n_chunks][cols][2] device: overflow blocks and body words per record
    unsigned* host_count = nullptr;           // the same, host-pinned (the task-queue kernel hands a finished chunk's counters over)
    unsigned long long stride = 0;
    unsigned cap = 0;                         // overflow blocks a record may hold
    int cols = 0;
    const int* pred = nullptr;                // [cols] device: Table::pred
    SIMPLYP_PACK_HD Layout layout_of(int E, int nd) const { return layout((size_t)E, nd, cap); }     // = Table::layout_of(c)
};

// One wavefront packs its block g of chunk c -- `nd` rows from d_begin on -- of every column of a [cols][rows][E] table.
__device__ __forceinline__ void pack_chunk(const double* table, int rows, int E, int d_begin, int nd, int g, int lane, const PackArgs& args,
                                           int c, unsigned long long* lds)
{
    const Layout L = args.layout_of(E, nd);
    for (int j = 0; j < args.cols; ++j) {
        const size_t rec = (size_t)c * (size_t)args.cols + (size_t)j;
        const int k = __builtin_amdgcn_readfirstlane(args.pred[j]);
        const double* x = k >= 0 ? table + ((size_t)k * (size_t)rows + (size_t)d_begin) * (size_t)E : nullptr;
        pack_block(table + ((size_t)j * (size_t)rows + (size_t)d_begin) * (size_t)E, x, (size_t)E, nd, E, g, lane,
                   args.buf + rec * args.stride, L, args.count + 2 * rec, lds);
    }
}
#endif

// ---- host half ----

#if defined(__x86_64__)
// MXCSR at its default (round to nearest, no flush to zero, denormals are not zero) for the life of the object: the encoder,
// the decoder and the decode threads hold one, so predict() rounds as the device does whatever the caller's thread had set.
struct FpDefault {
    unsigned saved;
    FpDefault() : saved(_mm_getcsr()) { _mm_setcsr(0x1F80u); }
    ~FpDefault() { _mm_setcsr(saved); }
    FpDefault(const FpDefault&) = delete;
    FpDefault& operator=(const FpDefault&) = delete;
};
#else
struct FpDefault {};
#endif

// The 64 z of one row of width w into the row's image (`w` words, zeroed by the caller).
inline void pack_row_host(const uint64_t* z, int w, uint64_t* image)
{
    for (int i = 0; i < GROUP; ++i) {
        const int bit = i * w, wi = bit >> 6, sh = bit & 63;
        if (!z[i]) continue;
        image[wi] |= z[i] << sh;
        if (sh + w > 64) image[wi + 1] |= z[i] >> (64 - sh);
    }
}

// The encoder in plain C++, block by block and span by span like the device's.  counts[0] = overflow blocks, counts[1] = the word
// cursor (which may pass the capacity; spans beyond it are not stored).
inline void encode_record_host(const double* rows, const double* xrows, size_t stride, int nd, size_t E, unsigned char* rec,
                               const Layout& L, uint64_t counts[2])
{
    FpDefault fp;
    (void)fp;
    const uint64_t* src = (const uint64_t*)rows;
    const uint64_t* xsrc = (const uint64_t*)xrows;
    const int G = (int)((E + GROUP - 1) / GROUP);
    memcpy(rec, src, E * sizeof(uint64_t));
    uint64_t* body = (uint64_t*)(rec + L.off_body);
    uint64_t n_big = 0, cursor = 0;
    // z[0]: previous day or first order, z[1]: second order (ratio columns only)
    static thread_local uint64_t z[2][SPAN][GROUP];
    for (int g = 0; g < G; ++g) {
        const size_t e0 = (size_t)g * GROUP;
        unsigned char* dir = rec + L.off_dir + (size_t)g * L.dir_stride;
        bool big = false;
        double rprev[GROUP] = {};
        for (int s = 0; s < L.n_spans; ++s) {
            const int d_first = 1 + s * SPAN, n = nd - d_first < SPAN ? nd - d_first : SPAN;
            int w[2][SPAN];
            uint64_t total[2] = {0, 0};
            bool span_big[2] = {false, false};
            for (int k = 0; k < n; ++k) {
                const size_t d = (size_t)(d_first + k);
                uint64_t any[2] = {0, 0};
                for (int i = 0; i < GROUP; ++i) {
                    const size_t e = e0 + (size_t)i;
                    uint64_t v[2] = {0, 0};
                    if (e < E) {
                        const uint64_t yp = src[(d - 1) * stride + e];
                        uint64_t p1 = yp, p2 = yp;
                        if (xsrc) {
                            double r1;
                            predict2(xsrc[d * stride + e], xsrc[(d - 1) * stride + e], yp, rprev[i], r1, p1, p2);
                            if (d == 1) p2 = p1;
                            rprev[i] = r1;
                        }
                        v[0] = encode(src[d * stride + e], p1);
                        v[1] = encode(src[d * stride + e], p2);
                    }
                    for (int o = 0; o < 2; ++o) { z[o][k][i] = v[o]; any[o] |= v[o]; }
                }
                for (int o = 0; o < 2; ++o) {
                    span_big[o] = span_big[o] || !fits(any[o]);
                    w[o][k] = width_of(any[o]);
                    total[o] += (uint64_t)w[o][k];
                }
            }
            const int o = (xsrc && total[1] < total[0] && !(span_big[1] && !span_big[0])) ? 1 : 0;
            big = big || span_big[o];
            const uint64_t base = cursor;
            cursor += total[o];
            if (base + total[o] > L.body_cap_words) continue;
            const uint32_t b32 = (uint32_t)base;
            memcpy(dir + (size_t)s * 4, &b32, 4);
            uint64_t* at = body + base;
            for (int k = 0; k < n; ++k) {
                dir[L.off_widths + (size_t)(d_first - 1 + k)] = (unsigned char)(w[o][k] | ((o && k == 0) ? ORDER2 : 0));
                memset(at, 0, (size_t)w[o][k] * 8);
                pack_row_host(z[o][k], w[o][k], at);
                at += w[o][k];
            }
        }
        if (big) ++n_big;
    }
    counts[0] = n_big;
    counts[1] = cursor;
}

inline uint64_t load64(const unsigned char* p) { uint64_t v; memcpy(&v, p, 8); return v; }

// The 64 z of a row of any width.  Value i sits at bit i * w: eight bytes from byte (i * w) >> 3, and a ninth where the value
// ends beyond them (w > 56 only).
inline void unpack_row_scalar(const unsigned char* row, int w, uint64_t* z)
{
    if (w == 0) { memset(z, 0, GROUP * sizeof(uint64_t)); return; }
    const uint64_t mask = w == 64 ? ~0ull : (1ull << w) - 1ull;
    for (int i = 0; i < GROUP; ++i) {
        const int bit = i * w, by = bit >> 3, sh = bit & 7;
        uint64_t v = load64(row + by) >> sh;
        if (sh + w > 64) v |= (uint64_t)row[by + 8] << (64 - sh);
        z[i] = v & mask;
    }
}

// One member of a ratio column's row: r_prev becomes this row's r1 whatever the order, so that a second-order span can
// follow a first-order one.
inline void finish_ratio(uint64_t& run, uint64_t z, uint64_t x, uint64_t x_prev, double& r_prev, bool order2)
{
    double r1;
    uint64_t p1, p2;
    predict2(x, x_prev, run, r_prev, r1, p1, p2);
    r_prev = r1;
    run = decode(z, order2 ? p2 : p1);
}

// out[i] = pred[i] + unzigzag(z[i]) for a whole block row; `z` becomes the row's values (the next row's previous day).
// r_prev[64] is the block's running ratio (ratio columns), order2 what the row's span says (false on a chunk's first delta row).
inline void finish_row_scalar(uint64_t* run, const uint64_t* z, const uint64_t* x, const uint64_t* x_prev, double* r_prev, bool order2, int n)
{
    if (x) for (int i = 0; i < n; ++i) finish_ratio(run[i], z[i], x[i], x_prev[i], r_prev[i], order2);
    else for (int i = 0; i < GROUP; ++i) run[i] = decode(z[i], run[i]);
}

inline void store_row(unsigned long long* out, const uint64_t* run, int n)
{
    for (int i = 0; i < n; ++i) __builtin_nontemporal_store((unsigned long long)run[i], out + i);
}

#if defined(__x86_64__)
// w <= 56: one unaligned 8-byte load per value, a shift by (i * w) & 7 and a mask; the shifts repeat every 8 values (w bytes).
__attribute__((target("avx2"))) inline void unpack_row_avx2(const unsigned char* row, int w, uint64_t* z)
{
    int o[8];
    long long s[8];
    for (int t = 0; t < 8; ++t) { o[t] = (t * w) >> 3; s[t] = (t * w) & 7; }
    const __m256i mask = _mm256_set1_epi64x((long long)((1ull << w) - 1ull));
    const __m256i s0 = _mm256_set_epi64x(s[3], s[2], s[1], s[0]), s1 = _mm256_set_epi64x(s[7], s[6], s[5], s[4]);
    for (int m = 0; m < 8; ++m) {
        const unsigned char* p = row + (size_t)m * (size_t)w;
        const __m256i a = _mm256_set_epi64x((long long)load64(p + o[3]), (long long)load64(p + o[2]), (long long)load64(p + o[1]),
                                            (long long)load64(p + o[0]));
        const __m256i b = _mm256_set_epi64x((long long)load64(p + o[7]), (long long)load64(p + o[6]), (long long)load64(p + o[5]),
                                            (long long)load64(p + o[4]));
        _mm256_storeu_si256((__m256i*)(z + m * 8), _mm256_and_si256(_mm256_srlv_epi64(a, s0), mask));
        _mm256_storeu_si256((__m256i*)(z + m * 8 + 4), _mm256_and_si256(_mm256_srlv_epi64(b, s1), mask));
    }
}

// The same arithmetic as finish_row_scalar, four values per turn.  _mm256_div_pd, _mm256_mul_pd, _mm256_add_pd and
// _mm256_sub_pd are the IEEE operations.
__attribute__((target("avx2"))) inline void finish_row_avx2(uint64_t* run, const uint64_t* z, const uint64_t* x, const uint64_t* x_prev,
                                                            double* r_prev, bool order2, int n)
{
    const __m256i one = _mm256_set1_epi64x(1), zero = _mm256_setzero_si256();
    const __m256i absmask = _mm256_set1_epi64x(0x7FFFFFFFFFFFFFFFll), expmask = _mm256_set1_epi64x(0x7FF0000000000000ll);
    int i = 0;
    const int n4 = x ? n / 4 * 4 : GROUP;
    for (; i < n4; i += 4) {
        const __m256i zz = _mm256_loadu_si256((const __m256i*)(z + i));
        const __m256i d = _mm256_xor_si256(_mm256_srli_epi64(zz, 1), _mm256_sub_epi64(zero, _mm256_and_si256(zz, one)));
        __m256i p = _mm256_loadu_si256((const __m256i*)(run + i));
        if (x) {
            const __m256d q = _mm256_div_pd(_mm256_castsi256_pd(p), _mm256_loadu_pd((const double*)(x_prev + i)));
            const __m256i pb = _mm256_castpd_si256(_mm256_mul_pd(_mm256_loadu_pd((const double*)(x + i)), q));
            const __m256i mag = _mm256_and_si256(pb, absmask);
            const __m256i bad = _mm256_or_si256(_mm256_cmpeq_epi64(mag, zero), _mm256_cmpeq_epi64(_mm256_and_si256(pb, expmask), expmask));
            p = _mm256_blendv_epi8(pb, p, bad);
            if (order2) {
                const __m256d slope = _mm256_sub_pd(_mm256_add_pd(q, q), _mm256_loadu_pd(r_prev + i));
                const __m256i pb2 = _mm256_castpd_si256(_mm256_mul_pd(_mm256_loadu_pd((const double*)(x + i)), slope));
                const __m256i mag2 = _mm256_and_si256(pb2, absmask);
                const __m256i bad2 = _mm256_or_si256(_mm256_cmpeq_epi64(mag2, zero), _mm256_cmpeq_epi64(_mm256_and_si256(pb2, expmask), expmask));
                p = _mm256_blendv_epi8(pb2, p, bad2);
            }
            _mm256_storeu_pd(r_prev + i, q);
        }
        _mm256_storeu_si256((__m256i*)(run + i), _mm256_add_epi64(p, d));
    }
    if (x) for (; i < n; ++i) finish_ratio(run[i], z[i], x[i], x_prev[i], r_prev[i], order2);
}

// The common row in one pass: a full block, 1 <= w <= 56, previous-day prediction, `out` 32-byte aligned.  unpack_row_avx2,
// finish_row_avx2 and store_row_avx2 without the trip of z through memory: run[i] += unzigzag(z[i]), streamed to out[i].
__attribute__((target("avx2"))) inline void decode_row_avx2(const unsigned char* row, int w, uint64_t* run, unsigned long long* out)
{
    int o[8];
    long long s[8];
    for (int t = 0; t < 8; ++t) { o[t] = (t * w) >> 3; s[t] = (t * w) & 7; }
    const __m256i mask = _mm256_set1_epi64x((long long)((1ull << w) - 1ull)), one = _mm256_set1_epi64x(1), zero = _mm256_setzero_si256();
    const __m256i s0 = _mm256_set_epi64x(s[3], s[2], s[1], s[0]), s1 = _mm256_set_epi64x(s[7], s[6], s[5], s[4]);
    for (int m = 0; m < 8; ++m) {
        const unsigned char* p = row + (size_t)m * (size_t)w;
        __m256i a = _mm256_set_epi64x((long long)load64(p + o[3]), (long long)load64(p + o[2]), (long long)load64(p + o[1]),
                                      (long long)load64(p + o[0]));
        __m256i b = _mm256_set_epi64x((long long)load64(p + o[7]), (long long)load64(p + o[6]), (long long)load64(p + o[5]),
                                      (long long)load64(p + o[4]));
        a = _mm256_and_si256(_mm256_srlv_epi64(a, s0), mask);
        b = _mm256_and_si256(_mm256_srlv_epi64(b, s1), mask);
        a = _mm256_xor_si256(_mm256_srli_epi64(a, 1), _mm256_sub_epi64(zero, _mm256_and_si256(a, one)));
        b = _mm256_xor_si256(_mm256_srli_epi64(b, 1), _mm256_sub_epi64(zero, _mm256_and_si256(b, one)));
        a = _mm256_add_epi64(a, _mm256_load_si256((const __m256i*)(run + m * 8)));
        b = _mm256_add_epi64(b, _mm256_load_si256((const __m256i*)(run + m * 8 + 4)));
        _mm256_store_si256((__m256i*)(run + m * 8), a);
        _mm256_store_si256((__m256i*)(run + m * 8 + 4), b);
        _mm256_stream_si256((__m256i*)(out + m * 8), a);
        _mm256_stream_si256((__m256i*)(out + m * 8 + 4), b);
    }
}

__attribute__((target("avx2"))) inline void store_row_avx2(unsigned long long* out, const uint64_t* run, int n)
{
    int i = 0;
    if (((uintptr_t)out & 31) == 0)
        for (; i + 4 <= n; i += 4) _mm256_stream_si256((__m256i*)(out + i), _mm256_loadu_si256((const __m256i*)(run + i)));
    for (; i < n; ++i) __builtin_nontemporal_store((unsigned long long)run[i], out + i);
}
#endif

// Members [e0, e1) of a landed record into `dst` (the column's first row of the chunk, `stride` doubles per row), written with
// non-temporal stores; e0 is a multiple of 64.  `xdst` is the predictor column's first row of the chunk in the same table,
// already decoded for these members (nullptr: previous day): its rows are read back from there.  The caller holds an FpDefault.
inline void decode_range(const unsigned char* rec, const Layout& L, int nd, size_t E, size_t e0, size_t e1, double* dst,
                         const double* xdst, size_t stride)
{
#if defined(__x86_64__)
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
#endif
    alignas(32) uint64_t run[GROUP], z[GROUP];
    alignas(32) double r_prev[GROUP];
    const unsigned char* body = rec + L.off_body;
    for (size_t b0 = e0; b0 < e1; b0 += GROUP) {
        const int n = (int)(e1 - b0 < (size_t)GROUP ? e1 - b0 : (size_t)GROUP);
        const unsigned char* dir = rec + L.off_dir + (b0 / GROUP) * L.dir_stride;
        memset(run, 0, sizeof(run));
        memcpy(run, rec + b0 * 8, (size_t)n * 8);
        unsigned long long* out = (unsigned long long*)dst + b0;
        const uint64_t* x = xdst ? (const uint64_t*)xdst + b0 : nullptr;
        store_row(out, run, n);
        const unsigned char* row = body;
        bool span_order2 = false;
        memset(r_prev, 0, sizeof(r_prev));
        for (int d = 1; d < nd; ++d) {
            if ((d - 1) % SPAN == 0) {
                uint32_t base;
                memcpy(&base, dir + (size_t)((d - 1) / SPAN) * 4, 4);
                row = body + (size_t)base * 8;
                span_order2 = (dir[L.off_widths + (size_t)(d - 1)] & ORDER2) != 0;
            }
            const int w = dir[L.off_widths + (size_t)(d - 1)] & (ORDER2 - 1);
            const bool order2 = span_order2 && d > 1;
            out += stride;
            const uint64_t* xd = x ? x + (size_t)d * stride : nullptr;
            const uint64_t* xp = x ? x + (size_t)(d - 1) * stride : nullptr;
#if defined(__x86_64__)
            if (have_avx2) {
                if (!x && n == GROUP && w >= 1 && w <= Z_BITS && ((uintptr_t)out & 31) == 0) {
                    decode_row_avx2(row, w, run, out);
                    row += (size_t)w * 8;
                    continue;
                }
                if (w == 0) memset(z, 0, sizeof(z));
                else if (w <= Z_BITS) unpack_row_avx2(row, w, z);
                else unpack_row_scalar(row, w, z);
                finish_row_avx2(run, z, xd, xp, r_prev, order2, n);
                store_row_avx2(out, run, n);
                row += (size_t)w * 8;
                continue;
            }
#endif
            unpack_row_scalar(row, w, z);
            finish_row_scalar(run, z, xd, xp, r_prev, order2, n);
            store_row(out, run, n);
            row += (size_t)w * 8;
        }
    }
}

}  // namespace simplyp_pack
