// prover_key_io.inc -- a prover's key as the CanonicalSerialize image of the reference's `ProvingKey` / `VerifyingKey` (keyfmt.hpp has the
// container; DESIGN.md section 4.13).  Member functions of ProverT (declared in prover.hip, which includes this file inside
// namespace mzk { namespace { ).  No kernels here: mzk_poly_degree_dev, mzk_fr_encode_dev, mzk_srs_serialize and the G1 encoder.

// mzk_prover_serialize_key / _vk.  Polynomial lengths are the degrees of the resident rows (from_coefficients_vec strips trailing zeros),
// the commitments are mzk_prover_vk_commitments', g is commit-key point 0, the commit key is its first n + 3 points (trim(n + 2)).
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::serialize(bool vk_only, uint32_t flags, uint64_t num_inputs, const uint8_t* h_bytes, const uint8_t* beta_h_bytes, bool is_merged,
        uint8_t* out, uint64_t capacity, uint64_t* out_len) {
    const Key& K = key();
    uint64_t srs_len = 0;
    ck(mzk_srs_len(K.srs, &srs_len));
    if (world > 1 && srs_len == hi - lo) fail(MZK_ERR_UNSUPPORTED, "the handle's commit key is a rank's slice of the SRS: it cannot be written as a key");
    const bool compressed = flags & MZK_SER_COMPRESSED;
    const uint64_t g1 = keyfmt::g1_record_bytes(CURVE, compressed), g2 = keyfmt::g2_record_bytes(CURVE, compressed);
    const int nfix = nsel + W + (ultra ? 4 : 0);
    std::vector<uint64_t> len(nfix, 0);
    if (!vk_only) {                                                // the lengths first: they decide the size
        Buf d_len;
        d_len.alloc(((size_t)nfix * 8 + EL - 1) / EL);
        for (int r = 0; r < nfix; r++) ck(mzk_poly_degree_dev(fix(r), n, static_cast<uint64_t*>(d_len.p) + r, S));
        sync_stream();
        ck(mzk_dev_download(len.data(), d_len.p, (size_t)nfix * 8));
    }
    const uint64_t vk_len = 8 + 8 + (8 + W * g1) + (8 + nsel * g1) + (8 + W * EL) + g1 + 2 * g2 + 1 + 1 + (ultra ? 4 * g1 : 0);
    uint64_t total = vk_len;
    if (!vk_only) {
        total += 8 + 8 + (8 + (n + 3) * g1) + 1;
        for (int r = 0; r < nfix; r++) total += 8 + len[r] * EL;
    }
    if (out_len) *out_len = total;
    if (!out) return;
    if (capacity < total) fail(MZK_ERR_INVALID_ARG, "capacity: the image takes " + std::to_string(total) + " bytes");
    if (!h_bytes || !beta_h_bytes) fail(MZK_ERR_INVALID_ARG, "h_bytes / beta_h_bytes: the G2 elements of the open key, as bytes of the image's mode");

    uint8_t* p = out;
    auto put_u64 = [&](uint64_t v) { for (int b = 0; b < 8; b++) *p++ = (uint8_t)(v >> (8 * b)); };
    Buf stage;                                                     // one row of records, aligned: the host assembles the image
    auto put_poly = [&](int r) {
        put_u64(len[r]);
        if (!len[r]) return;
        ck(mzk_fr_encode_dev(CURVE, fix(r), len[r], stage.p, S));
        sync_stream();
        ck(mzk_dev_download(p, stage.p, len[r] * EL));
        p += len[r] * EL;
    };
    if (!vk_only) {
        stage.alloc(n);
        put_u64((uint64_t)W);
        for (int i = 0; i < W; i++) put_poly(nsel + i);
        put_u64((uint64_t)nsel);
        for (int i = 0; i < nsel; i++) put_poly(i);
        put_u64(n + 3);
        ck(mzk_srs_serialize(K.srs, 0, n + 3, compressed ? MZK_SER_COMPRESSED : 0u, p));
        p += (n + 3) * g1;
    }
    // VerifyingKey
    std::vector<uint64_t> xy((size_t)(nsel + W) * PT), pl(4 * PT);
    vk_commitments(xy.data(), ultra ? pl.data() : nullptr);
    std::vector<uint8_t> rec((size_t)(nsel + W + 4) * g1);
    ck(mzk_ctx_g1_encode(CURVE, xy.data(), (uint64_t)(nsel + W), flags & MZK_SER_COMPRESSED, rec.data()));
    if (ultra) ck(mzk_ctx_g1_encode(CURVE, pl.data(), 4, flags & MZK_SER_COMPRESSED, rec.data() + (size_t)(nsel + W) * g1));
    put_u64(n);
    put_u64(num_inputs);
    put_u64((uint64_t)W);
    std::memcpy(p, rec.data() + (size_t)nsel * g1, (size_t)W * g1); p += (size_t)W * g1;          // (vk_commitments: selectors, then sigmas)
    put_u64((uint64_t)nsel);
    std::memcpy(p, rec.data(), (size_t)nsel * g1); p += (size_t)nsel * g1;
    put_u64((uint64_t)W);
    for (int i = 0; i < W; i++) {
        const auto c = h64::canonical(K.k[i]);
        for (int j = 0; j < 4; j++) put_u64(c[j]);
    }
    ck(mzk_srs_serialize(K.srs, 0, 1, compressed ? MZK_SER_COMPRESSED : 0u, p)); p += g1;
    std::memcpy(p, h_bytes, g2); p += g2;
    std::memcpy(p, beta_h_bytes, g2); p += g2;
    *p++ = is_merged ? 1 : 0;
    *p++ = ultra ? 1 : 0;
    if (ultra) { std::memcpy(p, rec.data() + (size_t)(nsel + W) * g1, 4 * g1); p += 4 * g1; }
    if (!vk_only) {
        *p++ = ultra ? 1 : 0;
        for (int i = 0; ultra && i < 4; i++) put_poly(nsel + W + i);
    }
    if ((uint64_t)(p - out) != total) fail(MZK_ERR_INVALID_ARG, "internal: the image's length differs from its computed size");
}

// MZK_KEY_CHECK_COMMITMENTS: the records of vk against this prover's own commitments, and vk.open_key.g against commit-key point 0
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::check_vk_records(const uint8_t* image, const mzk_key_layout_t& L, bool compressed, uint64_t* out_bad) {
    const uint64_t g1 = L.g1_record_bytes;
    const uint32_t mode = compressed ? MZK_SER_COMPRESSED : 0u;
    std::vector<uint64_t> xy((size_t)(nsel + W) * PT), pl(4 * PT);
    vk_commitments(xy.data(), ultra ? pl.data() : nullptr);
    std::vector<uint8_t> rec((size_t)(nsel + W + 4) * g1), g(g1);
    ck(mzk_ctx_g1_encode(CURVE, xy.data(), (uint64_t)(nsel + W), mode, rec.data()));
    if (ultra) ck(mzk_ctx_g1_encode(CURVE, pl.data(), 4, mode, rec.data() + (size_t)(nsel + W) * g1));
    auto differ = [&](uint64_t image_off, size_t rec_index) { return std::memcmp(image + image_off, rec.data() + rec_index * g1, g1) != 0; };
    auto bad = [&](const std::string& comm, const std::string& poly, uint64_t i) {
        if (out_bad) *out_bad = i;
        fail(MZK_ERR_ENCODING, comm + " does not commit " + poly);
    };
    for (int i = 0; i < nsel; i++)
        if (differ(L.selector_comms_off + i * g1, i)) bad(keyfmt::idx("vk.selector_comms", i), keyfmt::idx("selectors", i), i);
    for (int i = 0; i < W; i++)
        if (differ(L.sigma_comms_off + i * g1, nsel + i)) bad(keyfmt::idx("vk.sigma_comms", i), keyfmt::idx("sigmas", i), i);
    static const char* const TAB[4] = {"range_table", "key_table", "table_dom_sep", "q_dom_sep"};
    for (int i = 0; ultra && i < 4; i++)
        if (differ(L.plookup_comms_off + i * g1, nsel + W + i)) bad(std::string("vk.plookup_vk.") + TAB[i] + "_comm", std::string("plookup_pk.") + TAB[i] + "_poly", i);
    ck(mzk_srs_serialize(key().srs, 0, 1, mode, g.data()));
    if (std::memcmp(image + L.g_off, g.data(), g1) != 0) {
        if (out_bad) *out_bad = 0;
        fail(MZK_ERR_ENCODING, "vk.open_key.g is not commit_key point 0");
    }
}
