// merlin.cuh -- Keccak-f[1600], STROBE-128 as merlin cuts it (merlin src/strobe.rs) and merlin::Transcript, for the host and the device
// alike: the Fiat-Shamir code of the verifier -- one transcript per proof on the device (verifier.cuh, stage B), the batch challenge r on
// the host (mzk_batch_verify_challenge).
//
// The 200-byte state lives in 25 lanes that the CALLER owns (little-endian byte order inside a lane, FIPS 202 3.1.2), `stride` words
// apart: a device caller puts them in LDS, interleaved among the block's threads, because the running byte position indexes them
// dynamically and a private array indexed so goes to scratch; only the permutation works on a private, statically indexed copy.  Bytes
// are reached by shifts, never through a byte pointer, so the code does not depend on the host's endianness either.
// Compiles under a plain C++ compiler too (tools/host_pairing_check.cpp).
// Product code: not shared with oracle/.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MZK_MERLIN_HD __host__ __device__ inline
#define MZK_MERLIN_CALL __host__ __device__ __attribute__((noinline))   // the permutation: one copy per kernel, called from every absorb site
#else
#define MZK_MERLIN_HD inline
#define MZK_MERLIN_CALL inline
#endif

namespace mzk {
namespace merlin {

constexpr uint32_t STROBE_R = 166;                               // 200 - 2 * 16 (128-bit security) - 2
constexpr uint32_t F_I = 1, F_A = 2, F_C = 4, F_M = 16, F_K = 32;

MZK_MERLIN_HD uint64_t rotl64(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// FIPS 202 3.2-3.3: 24 rounds of theta, rho, pi, chi, iota on lanes a[x + 5 y]
MZK_MERLIN_HD void keccak_f1600(uint64_t* a) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                                 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                                 0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                                 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    for (int rnd = 0; rnd < 24; rnd++) {
        uint64_t c[5];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 25; y += 5) a[x + y] ^= d;
        }
        // rho and pi along the one cycle (x, y) -> (y, 2x + 3y) that starts at (1, 0): lane t of the cycle moves on, rotated by (t+1)(t+2)/2
        int x = 1, y = 0;
        uint64_t cur = a[1];
#pragma unroll
        for (int t = 0; t < 24; t++) {
            const int nx = y, ny = (2 * x + 3 * y) % 5;
            const uint64_t next = a[nx + 5 * ny];
            a[nx + 5 * ny] = rotl64(cur, ((t + 1) * (t + 2) / 2) % 64);
            cur = next;
            x = nx, y = ny;
        }
#pragma unroll
        for (int row = 0; row < 25; row += 5) {
            uint64_t t[5];
#pragma unroll
            for (int i = 0; i < 5; i++) t[i] = a[row + i];
#pragma unroll
            for (int i = 0; i < 5; i++) a[row + i] = t[i] ^ (~t[(i + 1) % 5] & t[(i + 2) % 5]);
        }
        a[0] ^= RC[rnd];
    }
}

// merlin::Transcript over the caller's 25 lanes
struct Transcript {
    uint64_t* st;                                                 // lane i at st[i * stride]: a block's transcripts interleave their lanes in LDS
    uint32_t stride, pos, begin, flags;

    MZK_MERLIN_HD void xor_byte(uint32_t i, uint32_t b) { st[(i >> 3) * stride] ^= (uint64_t)(b & 0xffu) << (8 * (i & 7)); }
    MZK_MERLIN_HD uint32_t take_byte(uint32_t i) {                // reads byte i and clears it (STROBE's squeeze overwrites with zero)
        const int s = 8 * (i & 7);
        const uint32_t b = (uint32_t)(st[(i >> 3) * stride] >> s) & 0xffu;
        st[(i >> 3) * stride] &= ~((uint64_t)0xff << s);
        return b;
    }
    MZK_MERLIN_CALL void permute() {
        xor_byte(pos, begin);
        xor_byte(pos + 1, 0x04);
        xor_byte(STROBE_R + 1, 0x80);
        uint64_t a[25];                                           // the permutation runs on a private copy: statically indexed, so registers
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] = st[i * stride];
        keccak_f1600(a);
#pragma unroll
        for (int i = 0; i < 25; i++) st[i * stride] = a[i];
        pos = begin = 0;
    }
    MZK_MERLIN_CALL void permute_plain() {                        // Keccak-f alone (the initial state of STROBE)
        uint64_t a[25];
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] = st[i * stride];
        keccak_f1600(a);
#pragma unroll
        for (int i = 0; i < 25; i++) st[i * stride] = a[i];
    }
    MZK_MERLIN_HD void absorb_byte(uint32_t b) {
        xor_byte(pos, b);
        if (++pos == STROBE_R) permute();
    }
    MZK_MERLIN_HD void absorb(const uint8_t* p, uint32_t n) { for (uint32_t i = 0; i < n; i++) absorb_byte(p[i]); }
    MZK_MERLIN_HD void absorb_u32le(uint32_t v) { for (int i = 0; i < 4; i++) absorb_byte(v >> (8 * i)); }
    MZK_MERLIN_HD void begin_op(uint32_t f) {                    // (merlin never continues an operation with other flags, nor uses F_T)
        const uint32_t prev = begin;
        begin = pos + 1;
        flags = f;
        absorb_byte(prev);
        absorb_byte(f);
        if ((f & (F_C | F_K)) && pos) permute();
    }
    // Strobe128::new(b"Merlin v1.0") and the dom-sep of Transcript::new(label)
    MZK_MERLIN_HD void init(uint64_t* lanes, uint32_t lane_stride, const char* label, uint32_t label_len) {
        st = lanes;
        stride = lane_stride;
        for (uint32_t i = 0; i < 25; i++) st[i * stride] = 0;
        const uint8_t head[6] = {1, STROBE_R + 2, 1, 0, 1, 96};
        for (uint32_t i = 0; i < 6; i++) xor_byte(i, head[i]);
        const char* ver = "STROBEv1.0.2";
        for (uint32_t i = 0; i < 12; i++) xor_byte(6 + i, (uint8_t)ver[i]);
        pos = begin = flags = 0;
        permute_plain();
        begin_op(F_M | F_A);
        const char* proto = "Merlin v1.0";
        for (uint32_t i = 0; i < 11; i++) absorb_byte((uint8_t)proto[i]);
        append_message("dom-sep", 7, (const uint8_t*)label, label_len);
    }
    // meta_ad(label) || meta_ad(len as u32 LE, more) || ad(msg): the head of an append; the caller may absorb() the message in pieces
    MZK_MERLIN_HD void append_begin(const char* label, uint32_t label_len, uint32_t msg_len) {
        begin_op(F_M | F_A);
        for (uint32_t i = 0; i < label_len; i++) absorb_byte((uint8_t)label[i]);
        absorb_u32le(msg_len);
        begin_op(F_A);
    }
    MZK_MERLIN_HD void append_message(const char* label, uint32_t label_len, const uint8_t* msg, uint32_t msg_len) {
        append_begin(label, label_len, msg_len);
        absorb(msg, msg_len);
    }
    MZK_MERLIN_HD void challenge_bytes(const char* label, uint32_t label_len, uint8_t* out, uint32_t n) {
        begin_op(F_M | F_A);
        for (uint32_t i = 0; i < label_len; i++) absorb_byte((uint8_t)label[i]);
        absorb_u32le(n);
        begin_op(F_I | F_A | F_C);
        for (uint32_t i = 0; i < n; i++) {
            out[i] = (uint8_t)take_byte(pos);
            if (++pos == STROBE_R) permute();
        }
    }
};

}  // namespace merlin
}  // namespace mzk
