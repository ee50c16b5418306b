// check.cuh -- where a witness fails: the device half of mzk_prover_check_witness (include/mzk.h).
//
//   Circuit::check_circuit_satisfiability           relation/src/constraint_system.rs:389-451
//   check_gate / check_range_gate                   constraint_system.rs:695-738, 602-618
//   merged_table_value / merged_lookup_wire_value   constraint_system.rs:1441-1480 (their coefficients in tau)
//
// The reference walks the gate list on the host; a caller of the round-level ABI holds arrays only.  Here every family is one
// pass over values that are resident anyway: the selectors' values on H (forward NTTs of the coefficient forms), the [5][n]
// table block of the proving key, the wire values, the wire-variable table.
//   gate    one thread per row evaluates the gate identity
//   lookup  a hash join on 5-element keys, the tau-free form of the Plookup argument: open addressing at load factor <= 1/4, the
//           slot holds the smallest table row with that key, the keys are recomputed from their sources (never stored)
//   copy    rep[var] = smallest cell of the variable, then every cell against its representative's 32 bytes
// Failing lanes are counted per wavefront (__ballot, 64 lanes): one atomicAdd of the popcount and one atomicMin of the lowest
// failing index per wave that has any, none at all in a clean wave.  Sums and minima of integers: exact whatever the order.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mzk.h"
#include "fp.cuh"
#include "plonk.cuh"
#include "plookup.cuh"

namespace mzk {

// words of the result block in device memory (u32): counters start at 0, the minima and the representative at 0xFFFFFFFF
enum CheckWord { CHK_GATE_CNT = 0, CHK_LOOKUP_CNT, CHK_COPY_CNT, CHK_KIND, CHK_GATE_MIN, CHK_LOOKUP_MIN, CHK_COPY_MIN, CHK_COPY_REP,
                 CHK_ROW_WIRES = 8 /* 6 x 8 words */, CHK_RESIDUAL = 56 /* 8 words */, CHK_WORDS = 64 };

struct GateCheckArgs {
    const uint32_t* sel;      // [13][n] selector values on H: q_lc[4], q_mul[2], q_hash[4], q_o, q_c, q_ecc
    const uint32_t* wire;     // [W][n]
    const uint32_t* pi;       // [n] public-input values on H, or NULL (all zero)
    uint32_t* res;            // CheckWord block
    unsigned long long n;
};

// `fail` of the lanes of one wavefront -> *cnt += failing lanes, *mn = min(*mn, lowest failing index).  The lanes of a wave hold
// increasing indices, so the lowest failing lane holds the wave's lowest failing index.  Every lane of the wave must arrive.
__device__ __forceinline__ void check_wave_report(bool fail, uint32_t idx, uint32_t* __restrict__ cnt, uint32_t* __restrict__ mn) {
    const unsigned long long failing = __ballot(fail);
    if (failing == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)failing) - 1) {
        atomicAdd(cnt, (uint32_t)__popcll(failing));
        atomicMin(mn, idx);
    }
}

// pi + q_c + sum q_lc[j] w_j + q_mul[0] w_0 w_1 + q_mul[1] w_2 w_3 + sum q_hash[j] w_j^5 + q_ecc w_0 w_1 w_2 w_3 w_4 - q_o w_4 on row i
// (check_gate, constraint_system.rs:695-738); a selector that is zero on the row is skipped before its products
template <class P>
__device__ __forceinline__ Fp<P> gate_residual(const GateCheckArgs& a, unsigned long long i) {
    using F = Fp<P>;
    auto q = [&](int j) { return load_fp<P>(a.sel + ((size_t)j * a.n + i) * 8); };
    F w[5];
#pragma unroll
    for (int j = 0; j < 5; j++) w[j] = load_fp<P>(a.wire + ((size_t)j * a.n + i) * 8);
    F acc = q(11);
    if (a.pi) acc = acc + load_fp<P>(a.pi + i * 8);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const F s = q(j);
        if (!s.is_zero()) acc = acc + s * w[j];
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const F s = q(4 + j);
        if (!s.is_zero()) acc = acc + s * w[2 * j] * w[2 * j + 1];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const F s = q(6 + j);
        if (!s.is_zero()) {
            const F w2 = sqr(w[j]);
            acc = acc + s * sqr(w2) * w[j];
        }
    }
    {
        const F s = q(12);
        if (!s.is_zero()) acc = acc + s * w[0] * w[1] * w[2] * w[3] * w[4];
    }
    {
        const F s = q(10);
        if (!s.is_zero()) acc = acc - s * w[4];
    }
    return acc;
}

template <class P>
__global__ __launch_bounds__(PLK_THREADS) void witness_gate_check_kernel(GateCheckArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    const bool fail = i < a.n && !gate_residual<P>(a, i).is_zero();
    check_wave_report(fail, (uint32_t)i, a.res + CHK_GATE_CNT, a.res + CHK_GATE_MIN);
}

// pi[rows[i]] = vals[i]: the public input on the rows the caller names (distinct rows: witness_check_run resolves repeats)
__global__ __launch_bounds__(PLK_THREADS) void witness_pi_scatter_kernel(const uint4* __restrict__ vals, const uint32_t* __restrict__ rows, unsigned long long count,
                                                                          uint4* __restrict__ pi) {
    const unsigned long long i = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    if (i >= count) return;
    const size_t r = rows[i];
    pi[2 * r] = vals[2 * i];
    pi[2 * r + 1] = vals[2 * i + 1];
}

// ---- lookup: hash join on (first, q dom_sep, q a0, q a1, q a2) ---------------------------------------------------------------
struct LookupCheckArgs {
    const uint32_t* wire;     // [6][n]
    const uint32_t* tab;      // [5][n] range, key, table_dom_sep, q_dom_sep, q_lookup on H (proving key)
    uint32_t* slots;          // open-addressing table: smallest table row with the slot's key, PLK_EMPTY when free
    uint32_t* res;
    unsigned long long n;
    uint32_t mask;            // slots - 1
};
struct LookupKey { uint4 w[10]; };

template <class P>
__device__ __forceinline__ void key_put(LookupKey& k, int at, const Fp<P>& v) {
    k.w[2 * at] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    k.w[2 * at + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
// the table side of row j: (range, q tds, q key, q w_3, q w_4), q = q_lookup[j]
template <class P>
__device__ __forceinline__ LookupKey lookup_table_key(const LookupCheckArgs& a, unsigned long long j) {
    auto t = [&](int r) { return load_fp<P>(a.tab + ((size_t)r * a.n + j) * 8); };
    auto w = [&](int r) { return load_fp<P>(a.wire + ((size_t)r * a.n + j) * 8); };
    const Fp<P> q = t(4);
    LookupKey k;
    key_put<P>(k, 0, t(0));
    key_put<P>(k, 1, q * t(2));
    key_put<P>(k, 2, q * t(1));
    key_put<P>(k, 3, q * w(3));
    key_put<P>(k, 4, q * w(4));
    return k;
}
// the lookup side of row i: (w_5, q qds, q w_0, q w_1, q w_2), q = q_lookup[i]
template <class P>
__device__ __forceinline__ LookupKey lookup_wire_key(const LookupCheckArgs& a, unsigned long long i) {
    auto t = [&](int r) { return load_fp<P>(a.tab + ((size_t)r * a.n + i) * 8); };
    auto w = [&](int r) { return load_fp<P>(a.wire + ((size_t)r * a.n + i) * 8); };
    const Fp<P> q = t(4);
    LookupKey k;
    key_put<P>(k, 0, w(5));
    key_put<P>(k, 1, q * t(3));
    key_put<P>(k, 2, q * w(0));
    key_put<P>(k, 3, q * w(1));
    key_put<P>(k, 4, q * w(2));
    return k;
}
__device__ __forceinline__ bool lookup_keys_equal(const LookupKey& x, const LookupKey& y) {
    bool eq = true;
#pragma unroll
    for (int e = 0; e < 5; e++) eq = eq && fr_words_equal(x.w[2 * e], x.w[2 * e + 1], y.w[2 * e], y.w[2 * e + 1]);
    return eq;
}
// restated in tests/plookup_cases.py, which aims keys at one probe chain: change both together
__device__ __forceinline__ uint32_t lookup_key_hash(const LookupKey& k) {
    uint32_t h = 0;
#pragma unroll
    for (int e = 0; e < 5; e++) h = (h ^ (h >> 15)) * 0x9E3779B1u + fr_words_hash(k.w[2 * e], k.w[2 * e + 1]);
    return h ^ (h >> 16);
}

// slots[h] = smallest table row holding that key.  A row equal to its predecessor is never the first occurrence (the padding of the
// table is one long run of (0, 0, 0, 0, 0)) and is skipped.
template <class P>
__global__ __launch_bounds__(PLK_THREADS) void witness_lookup_insert_kernel(LookupCheckArgs a) {
    const unsigned long long j = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    if (j >= a.n) return;
    const LookupKey k = lookup_table_key<P>(a, j);
    if (j > 0 && lookup_keys_equal(k, lookup_table_key<P>(a, j - 1))) return;
    uint32_t h = lookup_key_hash(k) & a.mask;
    for (uint32_t probe = 0; probe <= a.mask; probe++) {             // load factor <= 1/4: terminates long before the bound
        const uint32_t cur = atomicCAS(&a.slots[h], PLK_EMPTY, (uint32_t)j);
        if (cur == PLK_EMPTY) return;
        if (lookup_keys_equal(k, lookup_table_key<P>(a, cur))) { atomicMin(&a.slots[h], (uint32_t)j); return; }
        h = (h + 1) & a.mask;
    }
}

// row i < n - 1 fails iff no table row carries its key (row n - 1 is not looked up: constraint_system.rs:1390-1398)
template <class P>
__global__ __launch_bounds__(PLK_THREADS) void witness_lookup_probe_kernel(LookupCheckArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    bool fail = false;
    if (i + 1 < a.n) {
        const LookupKey k = lookup_wire_key<P>(a, i);
        uint32_t h = lookup_key_hash(k) & a.mask;
        fail = true;
        for (uint32_t probe = 0; probe <= a.mask; probe++) {
            const uint32_t cur = a.slots[h];
            if (cur == PLK_EMPTY) break;
            if (lookup_keys_equal(k, lookup_table_key<P>(a, cur))) { fail = false; break; }
            h = (h + 1) & a.mask;
        }
    }
    check_wave_report(fail, (uint32_t)i, a.res + CHK_LOOKUP_CNT, a.res + CHK_LOOKUP_MIN);
}

// ---- copy constraints: cells as wire * n + row, all of them below 2^32 ---------------------------------------------------------
// A few variables own most cells: the bench circuit's `zero` and `one` sit on millions of them.  With the plain pass -- every cell one
// atomicMin -- the check of the 2^20-gate UltraPlonk bench circuit took 49.5 ms with the table set, against 2.5 ms for the same witness
// as a vector, where this pass does not run (profiles/check_witness_time_plain_copy_pass.txt).  A cell that reads a representative at or below its own index has nothing to add -- rep[] only decreases, so a stale read
// costs one atomic, never a wrong minimum -- and a wave whose live lanes all hold one variable sends its lowest cell alone.
__global__ __launch_bounds__(PLK_THREADS) void witness_copy_rep_kernel(const uint32_t* __restrict__ vars, unsigned long long cells, uint32_t* rep) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    uint32_t v = 0;
    bool live = false;
    if (c < cells) {
        v = vars[c];
        live = __hip_atomic_load(&rep[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)c;
    }
    const unsigned long long mask = __ballot(live);
    if (mask == 0) return;
    const int leader = __ffsll((long long)mask) - 1;
    const uint32_t first = __shfl(v, leader);
    if (__all(!live || v == first)) {
        if ((int)(threadIdx.x & 63) == leader) atomicMin(&rep[v], (uint32_t)c);
    } else if (live) {
        atomicMin(&rep[v], (uint32_t)c);
    }
}
__global__ __launch_bounds__(PLK_THREADS) void witness_copy_check_kernel(const uint4* __restrict__ wire, const uint32_t* __restrict__ vars, unsigned long long cells,
                                                                          const uint32_t* __restrict__ rep, uint32_t* __restrict__ res) {
    const unsigned long long c = (unsigned long long)blockIdx.x * PLK_THREADS + threadIdx.x;
    bool fail = false;
    if (c < cells) {
        const size_t r = rep[vars[c]];
        fail = r != c && !fr_words_equal(wire[2 * c], wire[2 * c + 1], wire[2 * r], wire[2 * r + 1]);
    }
    check_wave_report(fail, (uint32_t)c, res + CHK_COPY_CNT, res + CHK_COPY_MIN);
}

// ---- the reported row: one thread.  kind = the first failing family in the order gate, lookup, copy; the W wire values of its
// row, the gate residual when the family is the gate, the representative of the failing cell when it is the copy family
template <class P>
__global__ void witness_report_kernel(GateCheckArgs a, int W, const uint32_t* __restrict__ vars, const uint32_t* __restrict__ rep) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t* res = a.res;
    uint32_t kind = MZK_CHECK_SATISFIED;
    unsigned long long row = 0;
    if (res[CHK_GATE_CNT]) { kind = MZK_CHECK_GATE; row = res[CHK_GATE_MIN]; }
    else if (res[CHK_LOOKUP_CNT]) { kind = MZK_CHECK_LOOKUP; row = res[CHK_LOOKUP_MIN]; }
    else if (res[CHK_COPY_CNT]) { kind = MZK_CHECK_COPY; row = res[CHK_COPY_MIN] % a.n; }
    res[CHK_KIND] = kind;
    if (res[CHK_COPY_CNT]) res[CHK_COPY_REP] = rep[vars[res[CHK_COPY_MIN]]];
    if (kind == MZK_CHECK_SATISFIED) return;
    for (int j = 0; j < W; j++) store_fp<P>(res + CHK_ROW_WIRES + 8 * j, load_fp<P>(a.wire + ((size_t)j * a.n + row) * 8));
    if (kind == MZK_CHECK_GATE) store_fp<P>(res + CHK_RESIDUAL, gate_residual<P>(a, row));
}

}  // namespace mzk
