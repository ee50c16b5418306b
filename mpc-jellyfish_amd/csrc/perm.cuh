// perm.cuh -- the wire permutation of a finalised circuit and its sigma values: the device half of mzk_plonk_wire_permutation_dev and
// mzk_plonk_sigma_values_dev (include/mzk.h).
//
//   compute_wire_permutation                                    relation/src/constraint_system.rs:743-778
//   compute_extended_id_permutation / compute_extended_permutation   constraint_system.rs:913-960
//
// Cells are numbered c = wire * n + row.  A variable on the cells c_0 < c_1 < .. < c_(m-1) gives next[c_i] = c_((i+1) mod m): a stable
// grouping of the cells by their variable index.  Least-significant-digit radix sort on the variable index, 8 bits a pass, the cell as
// payload, only as many passes as n_vars - 1 has digits:
//   perm_hist_kernel     block b counts the digits of ITS contiguous chunk of the input in LDS -> hist[digit][block]
//   perm_scan_kernel     exclusive prefix sums over hist read digit-major: where block b's entries of digit d start
//   perm_scatter_kernel  block b walks its chunk tile by tile in input order; inside a tile an entry's place among the entries of its
//                        digit comes from wavefront match masks (__ballot per digit bit) and a per-wave count table in LDS
//   perm_link_kernel     sorted position p -> next[cell_p] = cell_(p+1) inside a run of equal variables, the run's first cell at its end
// Nothing is ordered by an atomic: every destination is a sum of counts, so the output is a function of the input alone.  The match
// masks aggregate per wavefront before any shared counter is touched -- a run of one variable over millions of cells (the bench
// circuit's `zero`) is 64 equal digits per wave, one LDS add and no serialisation, and costs what any other input of that size costs.
// The only global atomics are the validation's count and minimum (integers: exact whatever the order).
#pragma once
#include <hip/hip_runtime.h>

#include "fp.cuh"

namespace mzk {

constexpr int PERM_THREADS = 256;                       // one tile: an entry per thread, 4 wavefronts of 64
constexpr int PERM_WAVES = PERM_THREADS / 64;
constexpr int PERM_RADIX = 256;
constexpr unsigned PERM_MAX_BLOCKS = 1024;              // hist is [256][blocks] u32: one block of perm_scan_kernel scans it

struct PermPass {
    const uint32_t* keys_in;       // variable index per entry
    const uint32_t* cells_in;      // NULL in the first pass: entry i is cell i
    uint32_t* keys_out;
    uint32_t* cells_out;
    uint32_t* hist;                // [PERM_RADIX][blocks]
    unsigned long long cells, chunk;   // entries; entries per block (a multiple of PERM_THREADS)
    unsigned blocks, shift;
};

// the lanes of this wavefront whose digit equals this lane's (inactive entries match nothing); every lane of the wave must arrive
__device__ __forceinline__ unsigned long long perm_match(uint32_t digit, bool live) {
    unsigned long long m = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const unsigned long long set = __ballot(live && ((digit >> b) & 1u));
        m &= ((digit >> b) & 1u) ? set : ~set;
    }
    return live ? m : 0ull;
}

// indices >= n_vars: their number and the lowest such cell (res[0], res[1]; res[1] starts at 0xFFFFFFFF)
__global__ __launch_bounds__(PERM_THREADS) void perm_validate_kernel(const uint32_t* __restrict__ vars, unsigned long long cells, unsigned long long n_vars,
                                                                     uint32_t* __restrict__ res) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    const bool bad = c < cells && (unsigned long long)vars[c] >= n_vars;
    const unsigned long long failing = __ballot(bad);
    if (failing == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)failing) - 1) {
        atomicAdd(&res[0], (uint32_t)__popcll(failing));
        atomicMin(&res[1], (uint32_t)c);
    }
}

__global__ __launch_bounds__(PERM_THREADS) void perm_hist_kernel(PermPass a) {
    __shared__ uint32_t cnt[PERM_RADIX];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long lo = (unsigned long long)blockIdx.x * a.chunk;
    const unsigned long long hi = lo + a.chunk < a.cells ? lo + a.chunk : a.cells;
    for (unsigned long long base = lo; base < hi; base += PERM_THREADS) {
        const unsigned long long i = base + threadIdx.x;
        const bool live = i < hi;
        const uint32_t d = live ? (a.keys_in[i] >> a.shift) & 0xFFu : 0u;
        const unsigned long long m = perm_match(d, live);
        if (live && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    a.hist[(size_t)threadIdx.x * a.blocks + blockIdx.x] = cnt[threadIdx.x];
}

// in place: hist[j] = sum of hist[0 .. j), j over the PERM_RADIX * blocks entries; one block of 1024 threads
__global__ __launch_bounds__(1024) void perm_scan_kernel(uint32_t* __restrict__ hist, unsigned total) {
    __shared__ uint32_t part[1024];
    const unsigned per = (total + 1023u) / 1024u;
    const unsigned lo = threadIdx.x * per < total ? threadIdx.x * per : total;
    const unsigned hi = lo + per < total ? lo + per : total;
    uint32_t s = 0;
    for (unsigned j = lo; j < hi; j++) s += hist[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned off = 1; off < 1024; off <<= 1) {                  // inclusive scan of the 1024 partial sums
        const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;
    for (unsigned j = lo; j < hi; j++) {
        const uint32_t v = hist[j];
        hist[j] = run;
        run += v;
    }
}

__global__ __launch_bounds__(PERM_THREADS) void perm_scatter_kernel(PermPass a) {
    __shared__ uint32_t wcnt[PERM_WAVES][PERM_RADIX];    // entries of digit d in wave w of the tile, then: where they go
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t next_of_digit = a.hist[(size_t)threadIdx.x * a.blocks + blockIdx.x];   // thread t keeps the running destination of digit t
    const unsigned long long lo = (unsigned long long)blockIdx.x * a.chunk;
    const unsigned long long hi = lo + a.chunk < a.cells ? lo + a.chunk : a.cells;
    for (unsigned long long base = lo; base < hi; base += PERM_THREADS) {
#pragma unroll
        for (int w = 0; w < PERM_WAVES; w++) wcnt[w][threadIdx.x] = 0;
        __syncthreads();
        const unsigned long long i = base + threadIdx.x;
        const bool live = i < hi;
        const uint32_t key = live ? a.keys_in[i] : 0u;
        const uint32_t cell = live ? (a.cells_in ? a.cells_in[i] : (uint32_t)i) : 0u;
        const uint32_t d = (key >> a.shift) & 0xFFu;
        const unsigned long long m = perm_match(d, live);
        const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));      // equal digits on lower lanes: earlier in the input
        if (live && before == 0) wcnt[wave][d] = (uint32_t)__popcll(m);
        __syncthreads();
        {
            uint32_t run = next_of_digit;
#pragma unroll
            for (int w = 0; w < PERM_WAVES; w++) {
                const uint32_t c = wcnt[w][threadIdx.x];
                wcnt[w][threadIdx.x] = run;
                run += c;
            }
            next_of_digit = run;
        }
        __syncthreads();
        if (live) {
            const uint32_t dst = wcnt[wave][d] + before;                                // < cells: a prefix sum of the counts of the same entries
            a.keys_out[dst] = key;
            a.cells_out[dst] = cell;
        }
        __syncthreads();
    }
}

// keys sorted (stably, so the cells of a run ascend); cells NULL: position p is cell p (no pass ran: one variable).
// The end of a run of more than one cell finds the run's start by binary search for its first position.
__global__ __launch_bounds__(PERM_THREADS) void perm_link_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ cells, unsigned long long count,
                                                                 uint32_t* __restrict__ next) {
    const unsigned long long p = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    if (p >= count) return;
    const uint32_t k = keys[p];
    auto cell_at = [&](unsigned long long q) { return cells ? cells[q] : (uint32_t)q; };
    unsigned long long to;
    if (p + 1 < count && keys[p + 1] == k) to = p + 1;
    else if (p == 0 || keys[p - 1] != k) to = p;
    else {
        unsigned long long lo = 0, hi = p - 1;                           // keys[hi] == k; the smallest q with keys[q] == k
        while (lo < hi) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (keys[mid] < k) lo = mid + 1; else hi = mid;
        }
        to = lo;
    }
    next[cell_at(p)] = cell_at(to);
}

// sigma[c] = k[next[c] / n] * w^(next[c] mod n): the extended permutation as field elements (constraint_system.rs:913-960);
// omega: the n powers of w (boundary form)
struct SigmaArgs {
    const uint32_t* next;
    const uint32_t* omega;
    uint32_t* out;
    unsigned long long cells;
    unsigned log_n;
    uint32_t k[6][8];
};
template <class P>
__global__ __launch_bounds__(PERM_THREADS) void perm_sigma_kernel(SigmaArgs a) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    if (c >= a.cells) return;
    const uint32_t t = a.next[c];
    const uint32_t wire = t >> a.log_n, row = t & ((1u << a.log_n) - 1u);
    if (wire >= 6) return;                                              // (a table that is not a permutation of the cells: nothing is read out of range)
    Fp<P> kv;
#pragma unroll
    for (int q = 0; q < 8; q++) kv.l[q] = a.k[wire][q];
    store_fp<P>(a.out + c * 8, kv * load_fp<P>(a.omega + (size_t)row * 8));
}

}  // namespace mzk
