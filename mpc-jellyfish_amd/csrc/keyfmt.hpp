// keyfmt.hpp -- the container of a serialized `ProvingKey` / `VerifyingKey` (ark-serialize 0.4 derive order),
// walked on the host: plain C++, no HIP, no allocation besides the error text.  It reads length prefixes and tags only -- never a field
// element or a point -- and never touches memory outside [bytes, bytes + len): every read goes through Walk::need, and a count is
// compared with (bytes left) / (record size), never multiplied, so a count of 2^64 - 1 is "truncated" and cannot wrap.
//
//   usize = u64 LE; bool = 1 byte, 0 or 1; Option<T> = bool, then T if 1; Vec<T> = u64 LE count, then the items
//   Fr = 32 B LE canonical; DensePolynomial = Vec<Fr>; Commitment = G1Affine (srs_io.cuh); G2 = opaque bytes (BLS12-381 96 / 192 B, BN254 64 / 128 B)
//   ProvingKey    sigmas: Vec<Poly>  selectors: Vec<Poly>  commit_key: Vec<G1>  vk: VerifyingKey  plookup_pk: Option<4 x Poly>
//   VerifyingKey  domain_size: usize  num_inputs: usize  sigma_comms: Vec<G1>  selector_comms: Vec<G1>  k: Vec<Fr>
//                 open_key: {g: G1, h: G2, beta_h: G2}  is_merged: bool  plookup_vk: Option<4 x G1>
// Product code: not shared with oracle/.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/mzk.h"

namespace mzk {
namespace keyfmt {

constexpr uint64_t FR_BYTES = 32;
inline uint64_t g1_record_bytes(int curve, bool compressed) { return (uint64_t)(curve == MZK_CURVE_BLS12_381 ? 48 : 32) * (compressed ? 1 : 2); }
inline uint64_t g2_record_bytes(int curve, bool compressed) { return (uint64_t)(curve == MZK_CURVE_BLS12_381 ? 96 : 64) * (compressed ? 1 : 2); }

struct Walk {
    const uint8_t* p;
    uint64_t len, off = 0;
    std::string err;                                             // empty while the image is well formed
    Walk(const uint8_t* bytes, uint64_t n) : p(bytes), len(n) {}
    bool ok() const { return err.empty(); }
    bool fail(const std::string& what) { if (err.empty()) err = what; return false; }
    // `bytes` more bytes of `field` exist from off on (off <= len always holds)
    bool need(uint64_t bytes, const std::string& field) {
        if (!ok()) return false;
        if (bytes > len - off) return fail("truncated in " + field + " at byte " + std::to_string(len));
        return true;
    }
    bool u64(uint64_t* v, const std::string& field) {
        if (!need(8, field)) return false;
        uint64_t r = 0;
        for (int b = 0; b < 8; b++) r |= (uint64_t)p[off + b] << (8 * b);
        off += 8;
        *v = r;
        return true;
    }
    bool tag(uint32_t* v, const std::string& field) {             // a bool, or the tag of an Option
        if (!need(1, field)) return false;
        const uint8_t t = p[off];
        if (t > 1) return fail(field + ": tag byte " + std::to_string(t) + " at byte " + std::to_string(off) + " is neither 0 nor 1");
        off += 1;
        *v = t;
        return true;
    }
    // `count` records of `rec` bytes: *at = their offset.  count <= (len - off) / rec, so count * rec cannot wrap
    bool records(uint64_t count, uint64_t rec, uint64_t* at, const std::string& field) {
        if (!ok()) return false;
        if (count > (len - off) / rec) return fail("truncated in " + field + " at byte " + std::to_string(len));
        *at = off;
        off += count * rec;
        return true;
    }
    bool poly(uint64_t* at, uint64_t* count, const std::string& field) {
        return u64(count, field + ".len") && records(*count, FR_BYTES, at, field);
    }
};

inline std::string idx(const char* name, uint64_t i) { return std::string(name) + "[" + std::to_string(i) + "]"; }

// the VerifyingKey at w.off; W / nsel: what the enclosing ProvingKey fixed, or 0 for a bare image (the counts of the vk decide)
inline bool walk_vk(Walk& w, int curve, bool compressed, uint32_t W, mzk_key_layout_t* o) {
    const uint64_t g1 = g1_record_bytes(curve, compressed), g2 = g2_record_bytes(curve, compressed);
    uint64_t cnt = 0;
    const bool bare = W == 0;
    o->vk_off = w.off;
    if (!w.u64(&o->domain_size, "vk.domain_size") || !w.u64(&o->num_inputs, "vk.num_inputs")) return false;
    const uint64_t n = o->domain_size;
    if (n == 0 || (n & (n - 1)) != 0) return w.fail("vk.domain_size: " + std::to_string(n) + " is not a power of two");
    if (n > (1ull << 27)) return w.fail("vk.domain_size: " + std::to_string(n) + " is above 2^27");
    if (!w.u64(&cnt, "vk.sigma_comms.len")) return false;
    if (W == 0) {
        if (cnt != 5 && cnt != 6) return w.fail("vk.sigma_comms: count " + std::to_string(cnt) + " is neither 5 nor 6");
        W = (uint32_t)cnt;
        o->num_wire_types = W;
        o->num_selectors = W == 6 ? 14 : 13;
    } else if (cnt != W) return w.fail("vk.sigma_comms: count " + std::to_string(cnt) + " does not match the " + std::to_string(W) + " sigma polynomials");
    if (!w.records(cnt, g1, &o->sigma_comms_off, "vk.sigma_comms")) return false;
    if (!w.u64(&cnt, "vk.selector_comms.len")) return false;
    if (cnt != o->num_selectors) return w.fail("vk.selector_comms: count " + std::to_string(cnt) + " does not match the " + std::to_string(o->num_selectors) + " selectors");
    if (!w.records(cnt, g1, &o->selector_comms_off, "vk.selector_comms")) return false;
    if (!w.u64(&cnt, "vk.k.len")) return false;
    if (cnt != W) return w.fail("vk.k: count " + std::to_string(cnt) + " does not match the " + std::to_string(W) + " wire types");
    if (!w.records(cnt, FR_BYTES, &o->k_off, "vk.k")) return false;
    if (!w.records(1, g1, &o->g_off, "vk.open_key.g") || !w.records(1, g2, &o->h_off, "vk.open_key.h") || !w.records(1, g2, &o->beta_h_off, "vk.open_key.beta_h"))
        return false;
    if (!w.tag(&o->is_merged, "vk.is_merged")) return false;
    uint32_t has = 0;
    if (!w.tag(&has, "vk.plookup_vk")) return false;
    o->has_plookup_vk = has;
    if (has && !w.records(4, g1, &o->plookup_comms_off, "vk.plookup_vk")) return false;
    if (bare && (W == 6) != (has != 0))                           // (inside a ProvingKey: judged with plookup_pk, once that tag is read)
        return w.fail(W == 6 ? "vk.plookup_vk: absent with 6 wire types" : "vk.plookup_vk: present with 5 wire types");
    o->vk_len = w.off - o->vk_off;
    return true;
}

// Fills *o (zeroed first) from the image; false: w.err names the field and the reason
inline bool walk(Walk& w, int curve, uint32_t flags, mzk_key_layout_t* o) {
    *o = mzk_key_layout_t{};
    const bool compressed = flags & MZK_SER_COMPRESSED;
    o->g1_record_bytes = g1_record_bytes(curve, compressed);
    o->g2_record_bytes = g2_record_bytes(curve, compressed);
    if (flags & MZK_KEY_VK_ONLY) {
        if (!walk_vk(w, curve, compressed, 0, o)) return false;
    } else {
        uint64_t cnt = 0;
        if (!w.u64(&cnt, "sigmas.len")) return false;
        if (cnt != 5 && cnt != 6) return w.fail("sigmas: count " + std::to_string(cnt) + " is neither 5 nor 6");
        const uint32_t W = (uint32_t)cnt;
        o->num_wire_types = W;
        for (uint32_t i = 0; i < W; i++)
            if (!w.poly(&o->sigma_off[i], &o->sigma_len[i], idx("sigmas", i))) return false;
        if (!w.u64(&cnt, "selectors.len")) return false;
        if (cnt != (W == 6 ? 14u : 13u))
            return w.fail("selectors: count " + std::to_string(cnt) + " is not " + (W == 6 ? "14" : "13") + " for " + std::to_string(W) + " wire types");
        o->num_selectors = (uint32_t)cnt;
        for (uint32_t i = 0; i < o->num_selectors; i++)
            if (!w.poly(&o->selector_off[i], &o->selector_len[i], idx("selectors", i))) return false;
        if (!w.u64(&o->commit_key_count, "commit_key.len")) return false;
        if (!w.records(o->commit_key_count, o->g1_record_bytes, &o->commit_key_off, "commit_key")) return false;
        if (!walk_vk(w, curve, compressed, W, o)) return false;
        uint32_t has = 0;
        if (!w.tag(&has, "plookup_pk")) return false;
        o->has_plookup = has;
        if ((has != 0) != (o->has_plookup_vk != 0)) return w.fail("plookup_pk and vk.plookup_vk are not both present or both absent");
        if ((W == 6) != (has != 0)) return w.fail(W == 6 ? "plookup_pk: absent with 6 wire types" : "plookup_pk: present with 5 wire types");
        static const char* const TABLES[4] = {"plookup_pk.range_table_poly", "plookup_pk.key_table_poly", "plookup_pk.table_dom_sep_poly", "plookup_pk.q_dom_sep_poly"};
        for (int i = 0; has && i < 4; i++)
            if (!w.poly(&o->table_off[i], &o->table_len[i], TABLES[i])) return false;
        // what needs the domain size, which the image states after the polynomials
        const uint64_t n = o->domain_size;
        for (uint32_t i = 0; i < W; i++)
            if (o->sigma_len[i] > n) return w.fail(idx("sigmas", i) + ": " + std::to_string(o->sigma_len[i]) + " coefficients, more than the domain size " + std::to_string(n));
        for (uint32_t i = 0; i < o->num_selectors; i++)
            if (o->selector_len[i] > n) return w.fail(idx("selectors", i) + ": " + std::to_string(o->selector_len[i]) + " coefficients, more than the domain size " + std::to_string(n));
        for (int i = 0; has && i < 4; i++)
            if (o->table_len[i] > n) return w.fail(std::string(TABLES[i]) + ": " + std::to_string(o->table_len[i]) + " coefficients, more than the domain size " + std::to_string(n));
        if (o->commit_key_count < n + 3)
            return w.fail("commit_key: " + std::to_string(o->commit_key_count) + " points, fewer than the domain size + 3 = " + std::to_string(n + 3));
    }
    if (!w.ok()) return false;
    if (w.off != w.len) return w.fail(std::to_string(w.len - w.off) + " bytes left over after the last field, at byte " + std::to_string(w.off));
    o->total_len = w.off;
    return true;
}

}  // namespace keyfmt
}  // namespace mzk
