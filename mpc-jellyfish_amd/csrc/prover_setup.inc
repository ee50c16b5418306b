// prover_setup.inc -- set-up (PlonkKzgSnark::preprocess's device half, snark.rs:529-617), commitments over one or several ranks, small helpers.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

// PlonkKzgSnark::preprocess's device half (snark.rs:529-617): coefficient forms resident, evaluations on the needed classes
template <class FrP, int CURVE>
ProverT<FrP, CURVE>::ProverT(int log_n_, int W_, const uint64_t* sel, const uint64_t* sig, const uint64_t* tab, uint64_t poly_len,
        const uint64_t* k_mont, uint64_t commit_key, uint64_t lagrange_key, const mzk_comm* cm, CoeffsAt at) {
    curve = CURVE; log_n = log_n_; W = W_; ultra = W_ == 6; nsel = ultra ? 14 : 13;
    rows = W + 2 + (ultra ? 3 : 0);
    n = 1ull << log_n; m = 8 * n;
    key_ = std::make_shared<Key>();
    Key& K = *key_;                                                // (the one place, with install / take_wire_variables, that writes the key part)
    K.srs = commit_key; K.srs_lagrange = lagrange_key;
    if (cm) { comm = *cm; rank = cm->rank; world = cm->world; }
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && (!comm.all_gather || !comm.barrier)))
        fail(MZK_ERR_INVALID_ARG, "mzk_comm: 0 <= rank < world, all_gather and barrier callbacks required");
    for (int i = 0; i < W; i++) K.k.push_back(load(k_mont + 4 * i));
    std::tie(lo, hi) = shard_range(n + 3, rank, world);            // the proving key keeps trim(n + 2) = n + 3 powers (snark.rs:535, 561)
    uint64_t srs_len = 0;
    ck(mzk_srs_len(K.srs, &srs_len));
    const bool sliced = world > 1 && srs_len == hi - lo;           // the key IS this rank's range of the SRS (mzk_srs_slice)
    if (sliced) key_first = lo;
    else if (srs_len < n + 3) fail(MZK_ERR_INVALID_ARG, "commit key too small: need domain size + 3 powers (srs.rs:88), or exactly this rank's point range");
    if (K.srs_lagrange) {
        ck(mzk_srs_len(K.srs_lagrange, &srs_len));
        if (sliced ? srs_len != hi - lo : srs_len < n + 3)
            fail(MZK_ERR_INVALID_ARG, "Lagrange-basis key: 2^log_n + 3 points (mzk_srs_lagrange_from_srs(.., log_n, 3)), sliced like the commit key");
    }
    const int nfix = nsel + W + (ultra ? 4 : 0);
    take_stream();
    K.fixed.alloc((size_t)nfix * n);
    ck(mzk_dev_memset(K.fixed.p, 0, (size_t)nfix * n * EL, S));
    sync_stream();                                                 // the uploads below are synchronous copies, not ordered after S
    auto fix = [&](int r) { return K.fixed.at((size_t)r * n); };
    auto up_rows = [&](int first, int cnt, const uint64_t* src) {
        if (at == COEFFS_ON_DEVICE) ck(mzk_dev_copy2d(fix(first), n * EL, src, poly_len * EL, poly_len * EL, (uint64_t)cnt, S));   // (complete before the call: mzk_prover_create_from_circuit)
        else if (poly_len == n) ck(mzk_dev_upload(fix(first), src, (size_t)cnt * n * EL));
        else for (int i = 0; i < cnt; i++) ck(mzk_dev_upload(fix(first + i), src + (size_t)i * poly_len * 4, poly_len * EL));
    };
    up_rows(0, nsel, sel);
    up_rows(nsel, W, sig);
    if (ultra) up_rows(nsel + W, 4, tab);
    if (at == COEFFS_ON_DEVICE) sync_stream();
    // The quotient has degree W (n + 1) + 2 (prover.rs:916-919).  Its W + 3 coefficients from X^(Wn) on are the top coefficients of
    // its numerator (mzk_plonk_quotient_top_dev, n > W + 2), so W of the 8 residue classes of the quotient domain determine the
    // rest -- 5 for TurboPlonk, 6 for UltraPlonk -- and only those are resident and evaluated; the polynomial so recovered has the
    // expected degree whatever the witness, which is why round 5 checks the quotient identity at zeta.  Tiny domains: W + 1 classes
    // with one spare coefficient above the expected degree (or an unsatisfied witness could not trip WrongQuotientPolyDegree), else all 8.
    K.use_top = n > (uint64_t)W + 2 && n >= 8;
    const uint32_t needed = K.use_top ? (uint32_t)W : (((uint64_t)W * (n + 1) + 2 < (uint64_t)(W + 1) * n - 1 && W + 1 <= 8) ? (uint32_t)W + 1 : 8u);
    for (uint32_t kc = 0; kc < needed; kc++) K.classes.push_back(kc);
    own = class_range(rank, world, needed);                        // contiguous blocks of ceil(needed / world); the last ranks may own none
    // a rank that owns no class still registers one (a key cannot be empty); it is never evaluated
    const std::vector<uint32_t> resident = own.empty() ? std::vector<uint32_t>{K.classes.back()} : own;
    alloc_workspace();
    // (last: were the constructor to throw after it, ~Key would release it with the members)
    ck(mzk_ctx_pk_register_chunked(CURVE, log_n, W, sel, sig, tab, poly_len, k_mont, resident.data(), (uint32_t)resident.size(), at == COEFFS_ON_DEVICE, &K.pk));
    K.w_n = root_of_unity<FrP>(log_n);
    K.gen = Fr::from_words(FrP::GENERATOR);
}

// mzk_prover_fork: a new slot on parent's key.  No SRS work, no NTT, no upload: the shape, a stream and the workspace the constructor above
// allocates.  Reads nothing of parent's that a proof in flight on it writes (its workspace, state, stage, timings).
template <class FrP, int CURVE>
ProverT<FrP, CURVE>::ProverT(const ProverT& parent) {
    if (parent.world > 1)
        fail(MZK_ERR_UNSUPPORTED, "mzk_prover_fork: a prover with an mzk_comm of world > 1 cannot be forked (two slots would interleave one communicator's collectives)");
    curve = parent.curve; log_n = parent.log_n; W = parent.W; ultra = parent.ultra; nsel = parent.nsel; n = parent.n; device = parent.device;
    rows = parent.rows; m = parent.m;
    lo = parent.lo; hi = parent.hi; key_first = parent.key_first; own = parent.own;
    key_ = parent.key_;
    take_stream();
    alloc_workspace();
}

template <class FrP, int CURVE>
ProverT<FrP, CURVE>::~ProverT() {
    (void)mzk_dev_sync();                                          // (the key part, once its last holder goes, does the same before it releases the key)
    if (copy_stream) (void)mzk_stream_destroy(copy_stream);
}

// a stream of the context (two per context, handed out in turn), made in one burst with the MSM's sort streams so that none of them
// shares a hardware queue with another (csrc/msm.hip sort_stream_init); the handle does not own it
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::take_stream() {
    static std::atomic<uint32_t> next_stream[16];                        // per logical device: its first handle takes stream 0, the next stream 1, ..
    int32_t dev_now = 0;
    ck(mzk_get_device(&dev_now));
    if (!std::getenv("MZK_PROVER_NULL_STREAM")) ck(mzk_ctx_prover_stream(next_stream[dev_now & 15]++, &S));
}

// the workspace of one proof in flight; the rounds allocate the rest on first use (wv, wit, vals_ext, qsum)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::alloc_workspace() {
    rem.alloc(key().classes.size() * n);                           // the remainders of ALL needed classes: own ones computed here, the others received
    top.alloc(16);
    slab.alloc((size_t)rows * (n + 3)); quot.alloc(m); coeff.alloc((size_t)(W + 1) * n);
    split.alloc((size_t)W * (n + 3)); lin.alloc(n + 4); batch.alloc(n + 4); opening.alloc(n + 3); shifted.alloc(n + 3); tmp.alloc(64); deg.alloc(1);
    if (ultra) { hh.alloc(2 * n); table.alloc(n); lookup.alloc(n); sorted.alloc(2 * n); }
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::hbm_bytes(uint64_t* fixed_b, uint64_t* pk_b, uint64_t* ws_b) {
    uint64_t ws = 0;
    for (const Buf* b : std::initializer_list<const Buf*>{&slab, &quot, &coeff, &split, &lin, &batch, &opening, &shifted, &hh, &table, &lookup, &sorted, &tmp, &deg, &rem, &wv, &wit, &top,
                         &vals_ext, &qsum, own_vars.p ? &own_vars : &key().vars})
        ws += b->bytes();
    if (fixed_b) *fixed_b = key().fixed.bytes();
    if (ws_b) *ws_b = ws;
    if (pk_b) ck(mzk_plonk_pk_hbm_bytes(key().pk, pk_b));
}

// of those bytes, the ones other living handles reach too: the key part (with its variable table, unless this handle uses one of its own)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::shared_hbm_bytes(uint64_t* shared_b, uint32_t* sharers) {
    const long holders = key_.use_count();
    uint64_t pk_b = 0;
    if (holders > 1) ck(mzk_plonk_pk_hbm_bytes(key().pk, &pk_b));
    if (shared_b) *shared_b = holders > 1 ? key().fixed.bytes() + pk_b + (own_vars.p ? 0 : key().vars.bytes()) : 0;
    if (sharers) *sharers = (uint32_t)holders;
}

// Jacobian sums of the coefficients [a, b) of every polynomial over the SRS points of the same indices
template <class FrP, int CURVE>
std::vector<uint64_t> ProverT<FrP, CURVE>::msm_partials(const std::vector<const void*>& polys, const std::vector<uint64_t>& lens, uint64_t a, uint64_t b,
        uint64_t key) {
    const uint32_t kp = (uint32_t)polys.size();
    std::vector<const void*> p(kp);
    std::vector<uint64_t> l(kp), off(kp), xyz((size_t)kp * 3 * QL);
    for (uint32_t i = 0; i < kp; i++) {
        const uint64_t s0 = std::min(a, lens[i]), s1 = std::min(b, lens[i]);
        p[i] = static_cast<const uint8_t*>(polys[i]) + s0 * EL;
        l[i] = s1 - s0;
        off[i] = (s1 > s0 ? s0 : a) - key_first;                     // (a sliced key starts at this rank's lo: a >= lo there)
    }
    ck(mzk_msm_batch_dev(key ? key : this->key().srs, kp, p.data(), l.data(), off.data(), 1, xyz.data(), S));
    return xyz;
}

// the ranks' partial sums -> the commitments, identical on every rank: all-gather of k x 144 B (96 B on BN254) through host
// memory and <= 8 EC additions per commitment on the host (mzk_g1_sum_jacobian) -- the "all-reduce of partial EC sums"
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::combine_partials(const std::vector<uint64_t>& part, uint64_t* out_xy) {
    const size_t kp = part.size() / (3 * QL), one = 3 * QL;
    if (world == 1) { ck(mzk_g1_jacobian_to_affine(CURVE, part.data(), kp, out_xy)); return; }
    std::vector<uint64_t> all((size_t)world * part.size());
    if (comm.all_gather(comm.ctx, part.data(), part.size() * 8, all.data())) fail(MZK_ERR_INVALID_ARG, "mzk_comm.all_gather failed");
    std::vector<uint64_t> sum(kp * one), col((size_t)world * one);
    for (size_t i = 0; i < kp; i++) {
        for (int g = 0; g < world; g++) std::memcpy(&col[g * one], &all[((size_t)g * kp + i) * one], one * 8);
        ck(mzk_g1_sum_jacobian(CURVE, col.data(), world, &sum[i * one]));
    }
    ck(mzk_g1_jacobian_to_affine(CURVE, sum.data(), kp, out_xy));
}

// ... of polynomials of which this rank holds ONLY the coefficients [lo, lo + lens[i])
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::commit_slices(const std::vector<const void*>& slices, const std::vector<uint64_t>& lens, uint64_t* out_xy) {
    const uint32_t kp = (uint32_t)slices.size();
    std::vector<uint64_t> off(kp, lo - key_first), xyz((size_t)kp * 3 * QL);
    ck(mzk_msm_batch_dev(key().srs, kp, slices.data(), lens.data(), off.data(), 1, xyz.data(), S));
    combine_partials(xyz, out_xy);
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::vk_commitments(uint64_t* out_xy, uint64_t* out_plookup_xy) {   // set-up work: over several ranks sharded by point range like every commitment
    std::vector<const void*> ptrs;
    std::vector<uint64_t> lens;
    const int cnt = nsel + W + (ultra && out_plookup_xy ? 4 : 0);
    for (int i = 0; i < cnt; i++) { ptrs.push_back(fix(i)); lens.push_back(n); }
    std::vector<uint64_t> xy((size_t)cnt * PT);
    for (int i = 0; i < cnt; i += W) {                                       // W at a time, like a round's commitments: set-up does not enlarge the MSM scratch the proofs need
        const int k = std::min(W, cnt - i);
        commit(std::vector<const void*>(ptrs.begin() + i, ptrs.begin() + i + k), std::vector<uint64_t>(lens.begin() + i, lens.begin() + i + k), &xy[(size_t)i * PT]);
    }
    std::memcpy(out_xy, xy.data(), (size_t)(nsel + W) * PT * 8);
    if (ultra && out_plookup_xy) std::memcpy(out_plookup_xy, &xy[(size_t)(nsel + W) * PT], 4 * PT * 8);
}

template <class FrP, int CURVE>
auto ProverT<FrP, CURVE>::evaluate(const void* d, uint64_t len, uint32_t batch_n, uint64_t stride, const Fr& x) -> std::vector<Fr> {
    std::vector<Fr> out(batch_n);
    ck(mzk_poly_eval_dev(CURVE, d, len, batch_n, stride, x.l, reinterpret_cast<uint64_t*>(out.data()), S));
    return out;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::lincomb(const std::vector<Term>& terms, void* out, uint64_t out_len) {
    std::vector<const void*> ptrs;
    std::vector<uint64_t> lens, sc;
    for (auto& t : terms) { ptrs.push_back(t.p); lens.push_back(t.len); for (int i = 0; i < 4; i++) sc.push_back(t.s.l[i]); }
    ck(mzk_poly_lincomb_dev(CURVE, (uint32_t)terms.size(), ptrs.data(), lens.data(), sc.data(), out, out_len, S));
}

// sum of any number of terms into `out` (one launch takes 32)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::lincomb_many(const std::vector<Term>& terms, void* out, uint64_t out_len) {
    constexpr size_t MAXT = 32;
    if (terms.size() <= MAXT) { lincomb(terms, out, out_len); return; }
    lincomb(std::vector<Term>(terms.begin(), terms.begin() + MAXT), out, out_len);
    for (size_t i = MAXT; i < terms.size(); i += MAXT - 1) {
        std::vector<Term> chunk{{Fr::one(), out, out_len}};
        chunk.insert(chunk.end(), terms.begin() + i, terms.begin() + std::min(terms.size(), i + MAXT - 1));
        lincomb(chunk, out, out_len);                              // elementwise: reading out[j] before writing it is safe
    }
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::mask(const std::vector<int>& slab_rows, const uint64_t* blinders, uint32_t n_blind) {      // prover.rs:463-486
    std::vector<void*> ptrs;
    for (int r : slab_rows) ptrs.push_back(row(r));
    ck(mzk_poly_mask_dev(CURVE, (uint32_t)ptrs.size(), ptrs.data(), n, n_blind, blinders, S));
}

template <class FrP, int CURVE>
const void* ProverT<FrP, CURVE>::one_dev() {                                            // the field's one (Montgomery), resident: tmp[1]
    if (!one_ready) {
        const Fr one = Fr::one();
        ck(mzk_dev_upload(tmp.at(1), one.l, EL));
        one_ready = true;
    }
    return tmp.at(1);
}

template <class FrP, int CURVE>
auto ProverT<FrP, CURVE>::download_fr(const void* d) -> Fr {
    Fr v;
    sync_stream();                                                 // (a synchronous copy is ordered after the null stream, not after S)
    ck(mzk_dev_download(v.l, d, EL));
    return v;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::set_wire_variables(const uint32_t* v, uint64_t nv) {
    const size_t cnt = (size_t)W * n;
    for (size_t i = 0; i < cnt; i++)
        if (v[i] >= nv) fail(MZK_ERR_INVALID_ARG, "wire_variables: variable index " + std::to_string(v[i]) + " >= number of variables " + std::to_string(nv));
    Buf fresh;
    fresh.alloc((cnt * 4 + EL - 1) / EL);
    ck(mzk_dev_upload(fresh.p, v, cnt * 4));
    install_wire_variables(fresh, nv);
}

// where a table becomes the handle's (mzk_prover_set_wire_variables, mzk_prover_derive_wire_variables): `fresh` leaves with the table it
// replaces, or empty.  A key with other holders is theirs too: the table is replaced for this handle alone (copy-on-write)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::install_wire_variables(Buf& fresh, uint64_t nv) {
    const bool sole = key_.use_count() == 1;
    sync_stream();                                                 // (what this handle has queued may still read the table that leaves)
    (sole ? key_->vars : own_vars).swap(fresh);
    (sole ? key_->n_vars : own_n_vars) = nv;
    if (sole && own_vars.p) { Buf().swap(own_vars); own_n_vars = 0; }   // (set while the key was shared; the handle is alone again)
}

// mzk_prover_derive_wire_variables: the table from the key's own sigma polynomials (plonk.hip plonk_derive_variables_dev, on the handle's
// stream, in the context's shared scratch).  It is written into memory of its own and installed once complete: an error leaves the handle as it was
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::derive_wire_variables(uint64_t* out_nv) {
    const size_t cnt = (size_t)W * n;
    Buf fresh;
    fresh.alloc((cnt * 4 + EL - 1) / EL);
    uint64_t nv = 0;
    ck(mzk_ctx_derive_variables(key().pk, fix(nsel), fresh.p, &nv, S));
    install_wire_variables(fresh, nv);
    if (out_nv) *out_nv = nv;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::get_wire_variables(uint32_t* out, uint64_t capacity, uint64_t* out_nv) {
    const size_t cnt = (size_t)W * n;
    if (!vars_dev()) fail(MZK_ERR_INVALID_ARG, "the handle has no wire-variable table (mzk_prover_set_wire_variables, mzk_prover_derive_wire_variables)");
    if (out && capacity < cnt) fail(MZK_ERR_INVALID_ARG, "capacity_cells < num_wire_types * domain size");
    if (out) {
        sync_stream();
        ck(mzk_dev_download(out, vars_dev(), cnt * 4));
    }
    if (out_nv) *out_nv = vars_n();
}

// the same table, resident already and validated where it was sorted (mzk_prover_create_from_circuit): the buffer changes hands
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::take_wire_variables(Buf& d_vars, uint64_t nv) {
    key_->vars.swap(d_vars);                                       // (at construction: the key has one holder)
    key_->n_vars = nv;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::poly_dev(uint32_t which, const void** out_p, uint64_t* out_len) {
    if (which > (uint32_t)W) fail(MZK_ERR_INVALID_ARG, "which: 0 .. W - 1 wire polynomials, W the permutation product");
    if (stage != CREATED && stage < R1) fail(MZK_ERR_STATE, "no proof in flight");
    *out_p = row((int)which);
    *out_len = which < (uint32_t)W ? n + 2 : n + 3;
}
