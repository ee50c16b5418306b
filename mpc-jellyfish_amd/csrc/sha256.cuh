// sha256.cuh -- SHA-256 (FIPS 180-4) for the host and the device alike, as the ADVZ VID scheme uses it (Advz<E, Sha256>, primitives/src/vid/advz.rs;
// DESIGN.md section 4.17): the Merkle tree over the storage nodes' evaluations on the device (vid.cuh), the payload commitment and the
// pseudorandom scalar on the host (vid.hip).
//   compress(h, w)     one block: w holds the 16 big-endian message words and is the ROLLING schedule -- w[t & 15] is overwritten by W_t, so the
//                      schedule never leaves its 16 registers; all 64 rounds are unrolled and every index is static.  Rotates are
//                      __builtin_rotateright32, which gfx950 issues as one v_alignbit_b32.  No LDS, no table in memory: K_t are literals.
//   Stream             the byte-granular hasher of the host entry points (mzk_sha256, the expander, the commitment digests)
//   expand_message_xmd RFC 9380 section 5.3.1 over SHA-256 with the length of Z_pad a parameter: ark-ff 0.4's DefaultFieldHasher sets the
//                      expander's block size to the bytes per field element (48), not SHA-256's 64 -- XMD_Z_PAD_ARK below, a recollection of
//                      that source, unpinned until a fixture from the reference exists
// The device kernels never go through bytes: their messages are whole words (vid.cuh), put into w with static indices.
// Compiles under a plain C++ compiler too.  Product code: not shared with oracle/.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MZK_SHA_HD __host__ __device__ __forceinline__
#else
#define MZK_SHA_HD inline
#endif

namespace mzk {
namespace sha256 {

constexpr uint32_t DIGEST_BYTES = 32, DIGEST_WORDS = 8, BLOCK_BYTES = 64;
constexpr uint32_t XMD_Z_PAD_RFC = 64;             // RFC 9380: s_in_bytes of SHA-256
constexpr uint32_t XMD_Z_PAD_ARK = 48;             // ark-ff 0.4 DefaultFieldHasher<Sha256, 128>: block_size = len_per_base_elem (see above)
constexpr uint32_t HASH_TO_FIELD_BYTES = 48;       // ceil((255 + 128) / 8) = ceil((254 + 128) / 8): both scalar fields

MZK_SHA_HD uint32_t rotr(uint32_t x, int n) { return __builtin_rotateright32(x, (uint32_t)n); }
MZK_SHA_HD uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

MZK_SHA_HD void init(uint32_t (&h)[8]) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

#define MZK_SHA_ROUND(a, b, c, d, e, f, g, h_, t, k)                                                          \
    do {                                                                                                      \
        if ((t) >= 16) {                                                                                      \
            const uint32_t w15 = w[((t) + 1) & 15], w2 = w[((t) + 14) & 15];                                  \
            w[(t) & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[((t) + 9) & 15] +                  \
                           (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));                                        \
        }                                                                                                     \
        const uint32_t t1 = h_ + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + (k) + w[(t) & 15]; \
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));         \
        d += t1;                                                                                              \
        h_ = t1 + t2;                                                                                         \
    } while (0)
#define MZK_SHA_ROUNDS8(t, k0, k1, k2, k3, k4, k5, k6, k7)  \
    MZK_SHA_ROUND(a, b, c, d, e, f, g, hh, (t) + 0, k0);    \
    MZK_SHA_ROUND(hh, a, b, c, d, e, f, g, (t) + 1, k1);    \
    MZK_SHA_ROUND(g, hh, a, b, c, d, e, f, (t) + 2, k2);    \
    MZK_SHA_ROUND(f, g, hh, a, b, c, d, e, (t) + 3, k3);    \
    MZK_SHA_ROUND(e, f, g, hh, a, b, c, d, (t) + 4, k4);    \
    MZK_SHA_ROUND(d, e, f, g, hh, a, b, c, (t) + 5, k5);    \
    MZK_SHA_ROUND(c, d, e, f, g, hh, a, b, (t) + 6, k6);    \
    MZK_SHA_ROUND(b, c, d, e, f, g, hh, a, (t) + 7, k7)

// h <- h + compression of one block; w (the 16 message words, big-endian values) is consumed
MZK_SHA_HD void compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    MZK_SHA_ROUNDS8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u);
    MZK_SHA_ROUNDS8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u);
    MZK_SHA_ROUNDS8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau);
    MZK_SHA_ROUNDS8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u);
    MZK_SHA_ROUNDS8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u);
    MZK_SHA_ROUNDS8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u);
    MZK_SHA_ROUNDS8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u);
    MZK_SHA_ROUNDS8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u);
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
#undef MZK_SHA_ROUNDS8
#undef MZK_SHA_ROUND

// The last block of a message of `total_bytes` bytes whose final block holds FILLED whole words in w[0 .. FILLED): 0x80, zeros and the bit
// length.  FILLED <= 13, so the length fits the same block (the tree's messages end at word 4, 8 or 12: vid.cuh).
template <int FILLED>
MZK_SHA_HD void finish_words(uint32_t (&h)[8], uint32_t (&w)[16], uint64_t total_bytes) {
    static_assert(FILLED >= 0 && FILLED <= 13, "the pad and the length share the block");
    w[FILLED] = 0x80000000u;
#pragma unroll
    for (int j = FILLED + 1; j < 14; j++) w[j] = 0u;
    w[14] = (uint32_t)((total_bytes * 8ull) >> 32);
    w[15] = (uint32_t)(total_bytes * 8ull);
    compress(h, w);
}

// SHA256(c0 || c1 || c2) of three digests held as the words of their bytes in memory (little-endian loads): a branch of the ternary tree
MZK_SHA_HD void hash_branch(const uint32_t (&c0)[8], const uint32_t (&c1)[8], const uint32_t (&c2)[8], uint32_t (&out)[8]) {
    uint32_t h[8], w[16];
    init(h);
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = bswap(c0[j]); w[8 + j] = bswap(c1[j]); }
    compress(h, w);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = bswap(c2[j]);
    finish_words<8>(h, w, 96);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = bswap(h[j]);
}

// ---- host: bytes in, bytes out -------------------------------------------------------------------------------------------------------
struct Stream {
    uint32_t h[8];
    uint8_t buf[BLOCK_BYTES];
    uint64_t len = 0;
    Stream() { init(h); }
    void block(const uint8_t* p) {
        uint32_t w[16];
        for (int j = 0; j < 16; j++) w[j] = (uint32_t)p[4 * j] << 24 | (uint32_t)p[4 * j + 1] << 16 | (uint32_t)p[4 * j + 2] << 8 | p[4 * j + 3];
        compress(h, w);
    }
    void update(const uint8_t* p, uint64_t n) {
        uint32_t fill = (uint32_t)(len % BLOCK_BYTES);
        len += n;
        if (fill) {
            const uint64_t take = n < BLOCK_BYTES - fill ? n : BLOCK_BYTES - fill;
            std::memcpy(buf + fill, p, take);
            p += take, n -= take, fill += (uint32_t)take;
            if (fill < BLOCK_BYTES) return;
            block(buf);
        }
        for (; n >= BLOCK_BYTES; p += BLOCK_BYTES, n -= BLOCK_BYTES) block(p);
        if (n) std::memcpy(buf, p, n);
    }
    void update_zeros(uint64_t n) {
        const uint8_t z[BLOCK_BYTES] = {0};
        for (; n; n -= (n < BLOCK_BYTES ? n : BLOCK_BYTES)) update(z, n < BLOCK_BYTES ? n : BLOCK_BYTES);
    }
    void finish(uint8_t* out32) {
        const uint64_t bits = len * 8;
        uint32_t fill = (uint32_t)(len % BLOCK_BYTES);
        buf[fill++] = 0x80;
        if (fill > 56) { std::memset(buf + fill, 0, BLOCK_BYTES - fill); block(buf); fill = 0; }
        std::memset(buf + fill, 0, 56 - fill);
        for (int j = 0; j < 8; j++) buf[56 + j] = (uint8_t)(bits >> (56 - 8 * j));
        block(buf);
        for (int j = 0; j < 8; j++) { out32[4 * j] = (uint8_t)(h[j] >> 24); out32[4 * j + 1] = (uint8_t)(h[j] >> 16); out32[4 * j + 2] = (uint8_t)(h[j] >> 8); out32[4 * j + 3] = (uint8_t)h[j]; }
    }
};

inline void digest(const uint8_t* msg, uint64_t len, uint8_t* out32) {
    Stream s;
    if (len) s.update(msg, len);
    s.finish(out32);
}

// RFC 9380 section 5.3.1 with H = SHA-256 and Z_pad of z_pad_len zero bytes.  false: out_len above 255 * 32 or 65535, or a DST above 255 bytes
// (the RFC hashes such a DST first; nobody here has one).
inline bool expand_message_xmd(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint32_t z_pad_len, uint8_t* out, uint64_t out_len) {
    const uint64_t ell = (out_len + DIGEST_BYTES - 1) / DIGEST_BYTES;
    if (ell > 255 || out_len > 65535 || dst_len > 255) return false;
    const uint8_t dst_tail = (uint8_t)dst_len, l_i_b[3] = {(uint8_t)(out_len >> 8), (uint8_t)out_len, 0};
    uint8_t b0[DIGEST_BYTES], bi[DIGEST_BYTES];
    Stream s0;
    s0.update_zeros(z_pad_len);
    if (len) s0.update(msg, len);
    s0.update(l_i_b, 3);
    if (dst_len) s0.update(dst, dst_len);
    s0.update(&dst_tail, 1);
    s0.finish(b0);
    for (uint64_t i = 1; i <= ell; i++) {
        uint8_t x[DIGEST_BYTES + 1];
        for (uint32_t j = 0; j < DIGEST_BYTES; j++) x[j] = i == 1 ? b0[j] : (uint8_t)(b0[j] ^ bi[j]);
        x[DIGEST_BYTES] = (uint8_t)i;
        Stream s;
        s.update(x, sizeof x);
        if (dst_len) s.update(dst, dst_len);
        s.update(&dst_tail, 1);
        s.finish(bi);
        const uint64_t at = (i - 1) * DIGEST_BYTES;
        std::memcpy(out + at, bi, out_len - at < DIGEST_BYTES ? out_len - at : DIGEST_BYTES);
    }
    return true;
}

}  // namespace sha256
}  // namespace mzk
