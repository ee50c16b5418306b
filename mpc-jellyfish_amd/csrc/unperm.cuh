// unperm.cuh -- from sigma back to the wire-variable table: the device half of mzk_plonk_sigma_decode_dev and
// mzk_plonk_variables_from_permutation_dev (include/mzk.h), the inverses of perm.cuh's two.
//
//   decode   sigma[c] = k_a w^b  ->  next[c] = a n + b.  A hash join of the W n probe keys against the W n identity values k_a w^b, which
//            are never materialised: a slot holds the CELL, and its 32-byte key is recomputed from k[] and the n powers of w where it is
//            compared (one multiplication).  Open addressing after plookup_hash_insert_kernel, load factor <= 1/2, full-key comparison.
//            All keys are distinct (else the cosets k_a H meet, which is reported), so no slot and no address is hot.  Which slot a cell
//            lands in depends on arrival order; what a probe finds does not.
//   label    next -> variables in canonical numbering: the variable of a cell is the number of cycle minima below its cycle's minimum.
//            unperm_mark_kernel     range check; mark[next[c]] = 1 (every writer stores the same word)
//            unperm_unmarked_kernel a cell nobody marked has no predecessor: with all entries in range, none such <=> a permutation
//            unperm_init_kernel     state[c] = (min, jump) = (c, next[c]) in one 8-byte word
//            unperm_round_kernel    (min, jump)[c] <- (min(min[c], min[jump[c]]), jump[jump[c]]): after r rounds min covers 2^r cells.  One
//                                   8-byte gather a round, double-buffered, one launch a round; a round that lowers no minimum is the last
//                                   (on a permutation: were a cycle longer than 2^r, the cell 2^r steps before its minimum would change)
//            unperm_count_kernel    minima (min[c] == c) per block of 256 cells -> totals, scanned by perm_scan_kernel (perm.cuh)
//            unperm_rank_kernel     a minimum's variable: its block's offset + the minima before it in the block (wave ballots)
//            unperm_spread_kernel   every other cell copies the variable of its minimum
// Nothing is ordered by an atomic and no id comes from a counter: the table is a function of `next` alone.  The work per round is one
// gather per cell whatever the cycle structure -- jump is a bijection of the cells in every round, so a cycle of millions of cells (the
// bench circuit's `zero`) has no hot address either; only the number of rounds, ceil(log2(longest cycle)), depends on the input.  The
// only global atomics are the validations' counts and minima (integers: exact whatever the order).
#pragma once
#include <hip/hip_runtime.h>

#include "fp.cuh"
#include "perm.cuh"
#include "plookup.cuh"

namespace mzk {

constexpr uint32_t UNPERM_EMPTY = 0xFFFFFFFFu;

struct DecodeArgs {
    const uint32_t* sigma;         // W n elements, wire-major
    const uint32_t* omega;         // the n powers of w
    uint32_t* slots;               // mask + 1 cells, UNPERM_EMPTY where free
    uint32_t* next;
    uint32_t* res;                 // [0] cells whose sigma is no identity value, [1] the lowest; [2] cells of colliding identity values, [3] the lowest
    unsigned long long cells;
    unsigned log_n;
    uint32_t mask;
    uint32_t k[6][8];
};

struct FrWords { uint4 lo, hi; };
template <class P>
__device__ __forceinline__ FrWords unperm_words(const Fp<P>& v) {
    return {make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]), make_uint4(v.l[4], v.l[5], v.l[6], v.l[7])};
}
// k_a w^b of the cell t = a n + b < W n
template <class P>
__device__ __forceinline__ FrWords unperm_identity(const DecodeArgs& a, uint32_t t) {
    const uint32_t wire = t >> a.log_n, row = t & ((1u << a.log_n) - 1u);
    Fp<P> kv;
#pragma unroll
    for (int q = 0; q < 8; q++) kv.l[q] = a.k[wire][q];
    return unperm_words<P>(kv * load_fp<P>(a.omega + (size_t)row * 8));
}

template <class P>
__global__ __launch_bounds__(PERM_THREADS) void unperm_insert_kernel(DecodeArgs a) {
    const unsigned long long t = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    if (t >= a.cells) return;
    const FrWords v = unperm_identity<P>(a, (uint32_t)t);
    uint32_t h = fr_words_hash(v.lo, v.hi) & a.mask;
    for (uint32_t probe = 0; probe <= a.mask; probe++) {              // load factor <= 1/2: terminates long before the bound
        const uint32_t cur = atomicCAS(&a.slots[h], UNPERM_EMPTY, (uint32_t)t);
        if (cur == UNPERM_EMPTY) return;
        const FrWords o = unperm_identity<P>(a, cur);
        if (fr_words_equal(v.lo, v.hi, o.lo, o.hi)) {                 // k_a w^b = k_a' w^b': the cosets are not disjoint
            atomicAdd(&a.res[2], 1u);
            atomicMin(&a.res[3], cur < (uint32_t)t ? cur : (uint32_t)t);
            return;
        }
        h = (h + 1) & a.mask;
    }
}

template <class P>
__global__ __launch_bounds__(PERM_THREADS) void unperm_probe_kernel(DecodeArgs a) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    bool bad = false;
    if (c < a.cells) {
        const uint4* s = reinterpret_cast<const uint4*>(a.sigma) + 2 * c;
        const uint4 v0 = s[0], v1 = s[1];
        uint32_t h = fr_words_hash(v0, v1) & a.mask, found = UNPERM_EMPTY;
        for (uint32_t probe = 0; probe <= a.mask; probe++) {
            const uint32_t cur = a.slots[h];
            if (cur == UNPERM_EMPTY) break;
            const FrWords o = unperm_identity<P>(a, cur);
            if (fr_words_equal(v0, v1, o.lo, o.hi)) { found = cur; break; }
            h = (h + 1) & a.mask;
        }
        bad = found == UNPERM_EMPTY;
        a.next[c] = bad ? (uint32_t)c : found;                        // (in range whatever happens: the caller fails the call)
    }
    const unsigned long long failing = __ballot(bad);
    if (failing == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)failing) - 1) {                  // the lowest failing lane holds the wave's lowest cell
        atomicAdd(&a.res[0], (uint32_t)__popcll(failing));
        atomicMin(&a.res[1], (uint32_t)c);
    }
}

// ---- labelling -----------------------------------------------------------------------------------------------------------------------
// res[0] entries >= cells, res[1] the lowest cell holding one; in-range entries mark their target
__global__ __launch_bounds__(PERM_THREADS) void unperm_mark_kernel(const uint32_t* __restrict__ next, unsigned long long cells, uint32_t* __restrict__ mark,
                                                                   uint32_t* __restrict__ res) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    bool bad = false;
    if (c < cells) {
        const uint32_t t = next[c];
        bad = (unsigned long long)t >= cells;
        if (!bad) mark[t] = 1u;
    }
    const unsigned long long failing = __ballot(bad);
    if (failing == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)failing) - 1) {                  // the lowest failing lane holds the wave's lowest cell
        atomicAdd(&res[0], (uint32_t)__popcll(failing));
        atomicMin(&res[1], (uint32_t)c);
    }
}
// res[2] cells that are the successor of no cell, res[3] the lowest
__global__ __launch_bounds__(PERM_THREADS) void unperm_unmarked_kernel(const uint32_t* __restrict__ mark, unsigned long long cells, uint32_t* __restrict__ res) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    const bool bad = c < cells && mark[c] == 0u;
    const unsigned long long failing = __ballot(bad);
    if (failing == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)failing) - 1) {                  // the lowest failing lane holds the wave's lowest cell
        atomicAdd(&res[2], (uint32_t)__popcll(failing));
        atomicMin(&res[3], (uint32_t)c);
    }
}

// state word: min in the low half, jump in the high half
__device__ __forceinline__ unsigned long long unperm_pack(uint32_t mn, uint32_t jump) { return (unsigned long long)jump << 32 | mn; }

__global__ __launch_bounds__(PERM_THREADS) void unperm_init_kernel(const uint32_t* __restrict__ next, unsigned long long cells, unsigned long long* __restrict__ state) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    if (c < cells) state[c] = unperm_pack((uint32_t)c, next[c]);
}
// changed: one word per round, zeroed by the host; every writer stores the same value
__global__ __launch_bounds__(PERM_THREADS) void unperm_round_kernel(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                                    unsigned long long cells, uint32_t* __restrict__ changed) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    bool lower = false;
    if (c < cells) {
        const unsigned long long s = in[c], t = in[s >> 32];
        const uint32_t mine = (uint32_t)s, theirs = (uint32_t)t;
        lower = theirs < mine;
        out[c] = unperm_pack(lower ? theirs : mine, (uint32_t)(t >> 32));
    }
    if (__ballot(lower) != 0 && (threadIdx.x & 63) == 0) *changed = 1u;
}

// minima among this block's 256 cells; mine: the minima on lower threads of the block
__device__ __forceinline__ uint32_t unperm_block_minima(bool is_min, uint32_t* wave_cnt /* LDS, PERM_WAVES words */, uint32_t& mine) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(is_min);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PERM_WAVES; w++) {
        const uint32_t n = wave_cnt[w];
        before += w < wave ? n : 0u;
        total += n;
    }
    mine = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    return total;
}
__global__ __launch_bounds__(PERM_THREADS) void unperm_count_kernel(const unsigned long long* __restrict__ state, unsigned long long cells, uint32_t* __restrict__ totals) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    __shared__ uint32_t wave_cnt[PERM_WAVES];
    uint32_t mine;
    const uint32_t total = unperm_block_minima(c < cells && (uint32_t)state[c] == (uint32_t)c, wave_cnt, mine);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}
// offs: the exclusive scan of totals
__global__ __launch_bounds__(PERM_THREADS) void unperm_rank_kernel(const unsigned long long* __restrict__ state, unsigned long long cells, const uint32_t* __restrict__ offs,
                                                                   uint32_t* __restrict__ vars) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    const bool is_min = c < cells && (uint32_t)state[c] == (uint32_t)c;
    __shared__ uint32_t wave_cnt[PERM_WAVES];
    uint32_t mine;
    (void)unperm_block_minima(is_min, wave_cnt, mine);
    if (is_min) vars[c] = offs[blockIdx.x] + mine;
}
// (reads the entries of minima, writes the others: no entry is both)
__global__ __launch_bounds__(PERM_THREADS) void unperm_spread_kernel(const unsigned long long* __restrict__ state, unsigned long long cells, uint32_t* vars) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PERM_THREADS + threadIdx.x;
    if (c >= cells) return;
    const uint32_t mn = (uint32_t)state[c];
    if (mn != (uint32_t)c) vars[c] = vars[mn];
}

}  // namespace mzk
