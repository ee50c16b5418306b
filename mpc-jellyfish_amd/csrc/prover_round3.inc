// prover_round3.inc -- round 3 (prover.rs:192-209, 512-673, 902-960): quotient by residue class, split, commitments.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

// this instance's quotient polynomial, 8n coefficients into `quot` (prover.rs:512-673 without the sum over instances)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::quotient(const Fr& alpha) {
    st.alpha = alpha;
    // per OWN class: fold mod X^n - h_k^n, size-n coset NTTs, the fused kernel, size-n inverse coset NTT -> t mod (X^n - h_k^n), straight
    // into this class's slot of `rem` (the rows of the slab are read, not overwritten)
    if (!own.empty())
        ck(mzk_plonk_quotient_chunked_flags_dev(key().pk, slab.p, n + 3, n + 3, st.pi_zero ? MZK_QUOTIENT_PI_ZERO : 0u, ultra ? st.tau.l : nullptr, alpha.l,
                                                st.beta.l, st.gamma.l, rem.at((size_t)own[0] * n), S));
    if (world > 1) {
        // THE one exchange (SURVEY.md 8(e).3)
        const uint32_t first = own.empty() ? 0u : own[0];
        if (comm.exchange_classes) {
            ck(mzk_dev_sync());
            if (comm.exchange_classes(comm.ctx, rem.p, n * EL, first, (uint32_t)own.size(), (uint32_t)key().classes.size())) fail(MZK_ERR_INVALID_ARG, "mzk_comm.exchange_classes failed");
        } else {
            // every rank pushes its class remainders into the same slots of every other rank's `rem`, device to device (xGMI peer
            // copies; n x 32 B per class and peer), then all ranks meet
            if ((int)peer_rem.size() != world) fail(MZK_ERR_STATE, "mzk_prover_set_peer_buffers has not been called");
            if (!own.empty())
                for (int q = 0; q < world; q++)
                    if (q != rank)
                        ck(mzk_dev_copy_peer(static_cast<uint8_t*>(peer_rem[q]) + (size_t)own[0] * n * EL, peer_dev[q], rem.at((size_t)own[0] * n), device,
                                             own.size() * n * EL, S));
            ck(mzk_dev_sync());
            if (comm.barrier(comm.ctx)) fail(MZK_ERR_INVALID_ARG, "mzk_comm.barrier failed");
        }
    }
    // the inverse Vandermonde per coefficient index (replicated: every rank needs the quotient's coefficients for the split)
    if (key().use_top) {
        ck(mzk_plonk_quotient_top_dev(key().pk, slab.p, n + 3, n + 3, alpha.l, st.beta.l, st.gamma.l, top.p, nullptr, S));
        ck(mzk_plonk_quotient_combine_top_dev(CURVE, log_n, key().classes.data(), (uint32_t)key().classes.size(), rem.p, top.p, (uint32_t)W + 3, quot.p, S));
    } else {
        ck(mzk_plonk_quotient_combine_classes_dev(CURVE, log_n, key().classes.data(), (uint32_t)key().classes.size(), rem.p, quot.p, S));
    }
}

// split_quotient_polynomial (prover.rs:902-960) of the 8n coefficients at `q` into this->split
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::split_quotient(const void* q, const uint64_t* b_quot) {
    const uint64_t expected = (uint64_t)W * (n + 1) + 2;                                                  // quotient_polynomial_degree
    // only what lies at and above the expected degree is scanned: its length must be exactly 1 (read after the commitments)
    ck(mzk_poly_degree_dev(static_cast<const uint8_t*>(q) + expected * EL, m - expected, static_cast<uint64_t*>(deg.p), S));
    ck(mzk_dev_download_async(stage_back.reserve(64), deg.p, 8, S));                                          // (page-locked: on the host by the time the commitments return)
    // one launch: the W slices, b_i as coefficient n + 2 of slice i < W - 1, t_i[0] -= b_{i-1}, zeros elsewhere (poly.cuh,
    // poly_split_quotient_kernel; rounds 1-5 first half: a fill, and per slice a copy, a scalar store and a one-element linear combination)
    ck(mzk_poly_split_quotient_dev(CURVE, q, n, (uint32_t)W, b_quot, split.p, n + 3, S));
    st.split_len.assign(W, n + 3);
    st.split_len[W - 1] = expected + 1 - (uint64_t)(W - 1) * (n + 2);
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round3(const std::vector<ProverBase*>& inst, const uint64_t* alpha_p, const uint64_t* blinders, uint64_t* out) {
    Tick tick(*this);
    if (world > 1 && inst.size() > 1) fail(MZK_ERR_UNSUPPORTED, "several instances over several ranks: not supported");
    const Fr alpha = load(alpha_p);
    const Fr a3 = alpha * alpha * alpha, a7 = a3 * a3 * alpha;
    std::vector<Term> qterms;
    st.bases.clear();
    Fr base = Fr::one();
    for (ProverBase* b : inst) {
        ProverT* p = static_cast<ProverT*>(b);
        p->need(p->ultra ? R2_5 : R2, R3, "round 3 follows round 2 (2.5 with Plookup) of every instance");
        p->quotient(alpha);
        qterms.push_back({base, p->quot.p, m});
        st.bases.push_back(base);
        base = base * (p->ultra ? a7 : a3);                         // prover.rs:661-669
        if (p != this) ck(mzk_stream_wait_stream(S, p->S));         // its quotient was computed on its own stream
    }
    const void* q = quot.p;
    if (inst.size() > 1) {                                          // the per-instance quotients are combined after their inverse NTTs (linear maps)
        if (!qsum.p) qsum.alloc(m);
        lincomb_many(qterms, qsum.p, m);
        q = qsum.p;
    }
    tick.mark("r3_quotient");
    split_quotient(q, blinders);
    tick.mark("r3_split");
    std::vector<const void*> p;
    for (int i = 0; i < W; i++) p.push_back(split.at((size_t)i * (n + 3)));
    commit(p, st.split_len, out);
    tick.mark("r3_commit");
    // quot_poly.degree() != expected_degree => WrongQuotientPolyDegree (prover.rs:915-918): the reference's only guard against an
    // unsatisfied witness; it can fire on the W + 1 / 8-class paths (tiny domains) only -- with the top coefficients taken from the
    // numerator the degree is right by construction and round 5 checks the identity at zeta.  (The commitments have synchronised the
    // stream; the 8 bytes are in page-locked host memory already.)
    sync_stream();
    const uint64_t tail = *static_cast<const volatile uint64_t*>(stage_back.p);                               // copied behind the degree scan, before the commitments
    for (ProverBase* b : inst) b->stage = R3;
    if (tail != 1) {
        const uint64_t expected = (uint64_t)W * (n + 1) + 2;
        for (ProverBase* b : inst) b->stage = CREATED;
        fail(MZK_ERR_WRONG_QUOTIENT_DEGREE, "WrongQuotientPolyDegree: quotient polynomial of degree " +
                 (tail ? std::to_string(expected + tail - 1) : "below " + std::to_string(expected)) + ", expected " + std::to_string(expected) +
                 " (the witness does not satisfy the circuit)");
    }
}
