// keccak_transcript.cuh -- Keccak-256 (sha3::Keccak256: rate 136, pad byte 0x01) over merlin.cuh's Keccak-f[1600] and the
// SolidityTranscript of plonk/src/transcript/solidity.rs:31-78 on top of it, for the host and the device alike: one transcript per proof on
// the device (verifier.cuh, stage B), single challenges and the batch challenge r on the host (mzk_solidity_challenge,
// mzk_batch_verify_challenge_t).
//   new(label)                 the label is dropped; transcript = empty, state = 64 zero bytes
//   append_message(label, m)   the label is dropped; transcript ||= m
//   get_and_append_challenge   state = keccak256(state || transcript || 0x00) || keccak256(state || transcript || 0x01);
//                              challenge = state[0..48] little-endian mod r.  The transcript is NOT cleared and the challenge NOT appended.
// The two digests of one challenge share every byte but the last: `state || transcript` is absorbed once up to its last full block, the 25
// lanes are kept, and the tail block is finished twice.  The message is read as 64-bit little-endian WORDS from a source the caller
// supplies (word(j) = bytes 8 j .. 8 j + 7), so whole lanes are XORed in with static indices and the sponge state stays in registers; only
// the tail block is put together from a masked word, the suffix and the pad.  Bytes are reached by shifts, never through a byte pointer
// into a lane.  Compiles under a plain C++ compiler too.
// Product code: not shared with oracle/.
#pragma once
#include <cstdint>

#include "merlin.cuh"

namespace mzk {
namespace keccak {

constexpr uint32_t RATE = 136, RATE_WORDS = 17;                  // 200 - 2 * 32
constexpr uint32_t STATE_BYTES = 64, STATE_WORDS = 8;            // the transcript's `state`, hashed in front of the transcript

// the full blocks of a message: block b is words 17 b .. 17 b + 16
template <class Src>
MZK_MERLIN_HD void absorb_blocks(uint64_t (&a)[25], const Src& src, uint64_t n_blocks) {
    for (uint64_t b = 0; b < n_blocks; b++) {
#pragma unroll
        for (int j = 0; j < (int)RATE_WORDS; j++) a[j] ^= src.word(b * RATE_WORDS + j);
        merlin::keccak_f1600(a);
    }
}
// The rest of a message of `len` bytes after its len / 136 full blocks, then the suffix byte (when has_suffix), then pad10*1 with the
// first pad byte 0x01.  One block, or two when the suffix takes byte 135: the pad is then 0x01 at byte 0 and 0x80 at byte 135 of a fresh
// block; when the suffix lands on byte 134 (or, without a suffix, the message ends at 135) the pad is the single byte 0x81.
// Bytes of src at and past `len` may hold anything: the last word is masked.
template <class Src>
MZK_MERLIN_HD void finish(uint64_t (&a)[25], const Src& src, uint64_t len, bool has_suffix, uint32_t suffix) {
    const uint64_t w0 = len / RATE * RATE_WORDS;
    const uint32_t rem = (uint32_t)(len % RATE), fw = rem >> 3, fb = rem & 7;
    const uint32_t pad = rem + (has_suffix ? 1 : 0);             // where 0x01 goes, counted from the start of the first tail block (<= 136)
    const uint32_t n_tail = pad == RATE ? 2 : 1;
    for (uint32_t t = 0; t < n_tail; t++) {
        const uint32_t base = t * RATE;
#pragma unroll
        for (int j = 0; j < (int)RATE_WORDS; j++) {              // static lane indices: every position is a comparison, not an address
            uint64_t v = 0;
            if (t == 0 && (uint32_t)j < fw) v = src.word(w0 + j);
            if (t == 0 && (uint32_t)j == fw && fb) v = src.word(w0 + j) & ((1ull << (8 * fb)) - 1);
            if (has_suffix && t == 0 && (uint32_t)j == fw) v ^= (uint64_t)(suffix & 0xffu) << (8 * fb);
            if (pad >= base && pad < base + RATE && (uint32_t)j == ((pad - base) >> 3)) v ^= 1ull << (8 * ((pad - base) & 7));
            if (t + 1 == n_tail && j == (int)RATE_WORDS - 1) v ^= 0x80ull << 56;
            a[j] ^= v;
        }
        merlin::keccak_f1600(a);
    }
}

// state (8 words, in and out) <- keccak256(m || 0) || keccak256(m || 1), m = the first `len` bytes of src (state || transcript, len >= 64)
template <class Src>
MZK_MERLIN_HD void solidity_digests(const Src& src, uint64_t len, uint64_t (&state)[STATE_WORDS]) {
    uint64_t a[25], b[25];
#pragma unroll
    for (int j = 0; j < 25; j++) a[j] = 0;
    absorb_blocks(a, src, len / RATE);
#pragma unroll
    for (int j = 0; j < 25; j++) b[j] = a[j];
    finish(a, src, len, true, 0);
    finish(b, src, len, true, 1);
#pragma unroll
    for (int j = 0; j < 4; j++) { state[j] = a[j]; state[4 + j] = b[j]; }
}

// a message in one or two byte ranges (the second follows the first): the words of the host entry points
struct ByteSrc {
    const uint8_t* p0;
    uint64_t n0;
    const uint8_t* p1;
    uint64_t n1;
    MZK_MERLIN_HD uint64_t word(uint64_t j) const {
        uint64_t v = 0;
        for (uint32_t s = 0; s < 8; s++) {
            const uint64_t i = 8 * j + s;
            if (i < n0) v |= (uint64_t)p0[i] << (8 * s);
            else if (i - n0 < n1) v |= (uint64_t)p1[i - n0] << (8 * s);
        }
        return v;
    }
};
MZK_MERLIN_HD void keccak256(const uint8_t* msg, uint64_t len, uint8_t* out32) {
    const ByteSrc src{msg, len, nullptr, 0};
    uint64_t a[25];
    for (int j = 0; j < 25; j++) a[j] = 0;
    absorb_blocks(a, src, len / RATE);
    finish(a, src, len, false, 0);
    for (int s = 0; s < 32; s++) out32[s] = (uint8_t)(a[s >> 3] >> (8 * (s & 7)));
}
// one get_and_append_challenge on the host: state64 (in, out) and the whole transcript so far; the challenge is state64[0..48] mod r
MZK_MERLIN_HD void solidity_squeeze_bytes(uint8_t* state64, const uint8_t* transcript, uint64_t len) {
    const ByteSrc src{state64, STATE_BYTES, transcript, len};
    uint64_t st[STATE_WORDS];
    solidity_digests(src, STATE_BYTES + len, st);
    for (uint32_t s = 0; s < STATE_BYTES; s++) state64[s] = (uint8_t)(st[s >> 3] >> (8 * (s & 7)));
}

// The transcript of one proof over words the CALLER owns, `stride` apart (a block's transcripts interleave their words in device memory, so
// a wave's loads of word j are one contiguous run): [ state, 8 words | transcript, up to cap - 8 words | MAX_CHALLENGES lengths ].
// Appends pack bytes into a word and store it whole; bytes past the capacity are dropped (the host sizes the slot from the key's shape and
// the longest extra message, so none are).  A challenge only RECORDS the length of the transcript at that point: squeeze_all() then hashes
// the recorded prefixes one after the other, in one loop around one inlined copy of the hash -- no call, so the 25 lanes stay in registers
// and nothing of the caller's is live across it.  The interface is merlin::Transcript's where the verifier's append code meets it.
constexpr uint32_t MAX_CHALLENGES = 8;
struct SolidityTranscript {
    uint64_t* w;
    uint64_t cur;                                                 // the word being filled
    uint32_t stride, cap, n, n_marks;                             // cap: words of state and transcript; n: bytes so far, the 64 of the state included

    static MZK_MERLIN_HD uint32_t slot_words(uint64_t transcript_bytes) { return (uint32_t)((STATE_BYTES + transcript_bytes + 7) / 8 + 1 + MAX_CHALLENGES); }
    MZK_MERLIN_HD void init(uint64_t* words, uint32_t word_stride, uint32_t n_slot_words) {
        w = words, stride = word_stride, cap = n_slot_words - MAX_CHALLENGES, n = STATE_BYTES, n_marks = 0, cur = 0;
        for (uint32_t j = 0; j < STATE_WORDS; j++) w[j * stride] = 0;
    }
    MZK_MERLIN_HD void absorb_byte(uint32_t b) {
        if (n >= 8 * cap) return;
        cur |= (uint64_t)(b & 0xffu) << (8 * (n & 7));
        if ((++n & 7) == 0) { w[((n >> 3) - 1) * stride] = cur; cur = 0; }
    }
    MZK_MERLIN_HD void absorb(const uint8_t* p, uint32_t len) { for (uint32_t i = 0; i < len; i++) absorb_byte(p[i]); }
    MZK_MERLIN_HD void append_begin(const char*, uint32_t, uint32_t) {}                       // labels and lengths are not hashed
    MZK_MERLIN_HD void append_message(const char*, uint32_t, const uint8_t* msg, uint32_t len) { absorb(msg, len); }
    MZK_MERLIN_HD void mark() {                                   // get_and_append_challenge, deferred: challenge n_marks hashes the first n bytes
        if (n_marks < MAX_CHALLENGES) w[(cap + n_marks++) * stride] = n;
    }
    MZK_MERLIN_HD uint64_t word(uint64_t j) const { return w[j * stride]; }
    // every recorded challenge in order: out(k, state) with the new state, whose first 48 bytes are the challenge (state[0..5])
    template <class Out>
    MZK_MERLIN_HD void squeeze_all(Out&& out) {
        if (n & 7) w[(n >> 3) * stride] = cur;                    // (n < 8 cap here: the word exists)
#pragma unroll 1
        for (uint32_t k = 0; k < n_marks; k++) {
            uint64_t st[STATE_WORDS];
            solidity_digests(*this, w[(cap + k) * stride], st);
#pragma unroll
            for (int j = 0; j < (int)STATE_WORDS; j++) w[(uint32_t)j * stride] = st[j];
            out(k, st);
        }
    }
};

}  // namespace keccak
}  // namespace mzk
