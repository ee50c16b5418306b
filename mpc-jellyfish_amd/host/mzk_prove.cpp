// mzk_prove -- PlonkKzgSnark::prove on the reference's bench circuit from a compiled host: C++ above the C ABI of
// include/mzk.h, no Python, no HIP in this translation unit (g++ builds it).
//   mzk_prove <curve: 0 BLS12-381 | 1 BN254> <turbo|ultra> <num_gates> [reps] [range_bit_len] [--gpus G] [--transcript merlin|solidity] [--host-witness | --host-witness-vars] [--check-agree]
//   mzk_prove <curve> file <circuit file> [reps] [--gpus G] [--host-witness] ...
// --check-witness (turbo, ultra, file): mzk_prover_check_witness before proving; prints one line -- `witness: satisfied`, or
// `witness: gate row R residual 0x..`, `witness: lookup row R`, `witness: copy cell (wire,row) != (wire,row)` -- followed by the numbers of
// failing gate rows, lookup rows and copy cells, and exits with status 3 without proving when the witness is not satisfied (--gpus G: rank 0 checks).
// --derive-variables (turbo, ultra, file): mzk_prover_derive_wire_variables after the set-up -- the wire-variable table recovered from the key's
// sigma polynomials, so that --check-witness checks the copy constraints of a prover that came from coefficient forms (a circuit file
// holds sigma values, not variables); when the first failing family is not the copy family, the first failing copy cell follows the counts.
// Not with --host-witness-vars: that witness vector is in the circuit's numbering, the derived table in the canonical one.
// --save-pk FILE (turbo, ultra, file; with --device-preprocess too): after the set-up the key is written as the CanonicalSerialize image of
// the reference's `ProvingKey` (mzk_prover_serialize_key; compressed unless --pk-uncompressed; h and beta_h of the open key are zero bytes:
// this host's testing setup has no G2 side).  --pk FILE (file): the proving key is read from such an image in place of the circuit file's
// selector and sigma values (mzk_prover_create_serialized, the commit key being this host's: the embedded points are skipped); the witness
// and the public input still come from the circuit file.  --pk-check: MZK_KEY_CHECK_COMMITMENTS.  --pk combines with --check-witness
// --derive-variables.  The JSON line carries pk_bytes: the size of the image written or read (0: neither).
// --srs FILE (turbo, ultra, file): commit over the powers of a setup file -- CanonicalSerialize of UnivariateUniversalParams, compressed --
// decoded and validated on every device, instead of the testing SRS [beta^i] G.  The trapdoor is still drawn (and discarded) from the rng,
// so the blinders are those of a run without --srs.  A file with fewer than n + 3 powers is an error.
// `file`: ANY finalised circuit -- public inputs, every gate type, copy constraints, lookups -- as the arrays `Arithmetization` exposes
// (format: BenchCircuitHost::read in mzk_prover.hpp; mpc-jellyfish_amd/circuit_io.py writes it).
// Prints one JSON line: proof bytes (hex), wall time per proof, per-round times of one profiled proof.
// --gpus G: G devices driven from this ONE process, one host thread per device (ShardedProver, mzk_prover.hpp): commitments sharded by
// point range, the quotient by residue class with one device-to-device exchange, rounds 4-5 by coefficient range; same proof bytes.
// With MZK_VIRTUAL_DEVICES=G in the environment the G device contexts share one card (rehearsal on a one-GPU box).
// --slots K (turbo, ultra; one device): K host threads prove `reps` proofs each on ONE proving key through K slots -- the prover and K - 1
// forks of it (mzk_prover_fork) -- and one JSON line reports proofs per second (against one slot alone), the family's HBM from
// mzk_prover_hbm_bytes / mzk_prover_shared_hbm_bytes, and with --check-agree whether every proof equals the one a single slot makes
// from the same rng seed.
//   mzk_prove <curve> link <num_gates_1> <num_gates_2> <alignment> <offset> <size> [reps]
//   mzk_prove <curve> batch <turbo|ultra> <range_bit_len> <num_gates_1> <num_gates_2> ...
// PlonkKzgSnark::batch_prove: one aggregated BatchProof over bench circuits of one domain size; prints its bytes.
// (link:) proves two TurboPlonk bench circuits of one domain size (wire 0 of the bench circuit holds 0, 1, 2, .. so any rows below both
// gate counts are shared witnesses), then PlonkKzgSnark::link_proofs on their hints; prints both proofs and the LinkingProof.
#include <chrono>
#include <cstdlib>
#include <memory>

#include <algorithm>
#include "mzk_prover.hpp"

using namespace mzk_host;

struct Options {
    int gpus = 1;                 // --gpus G: G devices from this one process, one host thread each (MZK_VIRTUAL_DEVICES=G: all on one card)
    int host_witness = 0;         // --host-witness: every proof uploads its W x n wire values from page-locked host memory;
                                  // --host-witness-vars: only the witness vector, gathered per wire on the device
    bool check_agree = false;     // --check-agree: every rank's proof bytes are compared (tests)
    TranscriptKind transcript = TranscriptKind::Merlin;  // --transcript merlin|solidity: the Fiat-Shamir transcript of every route (solidity: Keccak-256,
                                  // plonk/src/transcript/solidity.rs, for proofs a keccak256 verifier checks)
    int slots = 0;                // --slots K: K threads on one key through K slots (run_slots)
    const char* srs_path = nullptr;  // --srs FILE: the commit key from a serialized setup
    bool slice_srs = true;        // --no-slice: with --gpus G every rank keeps the whole commit key (and its table) instead of its point range
    bool device_preprocess = false;  // --device-preprocess: the proving key from the circuit's selector values and variable table, permutation and
                                  // sigma values on the device (mzk_prover_create_from_circuit_dev) -- same key, same bytes; bench circuits only
    bool derive_variables = false;  // --derive-variables: the wire-variable table from the key's sigma polynomials (mzk_prover_derive_wire_variables)
    bool check_witness = false;   // --check-witness: say where the witness fails before proving; exit status 3 if it does
    const char* pk_path = nullptr;   // --pk FILE (file): the proving key from the reference's serialized ProvingKey in place of the circuit file's selector
                                  // and sigma values; the witness and the public input still come from the circuit file
    const char* save_pk_path = nullptr;  // --save-pk FILE: the key as that image, after any preprocess (h and beta_h of the open key: zero bytes)
    bool pk_uncompressed = false; // --pk-uncompressed: the mode of both
    bool pk_check = false;        // --pk-check: MZK_KEY_CHECK_COMMITMENTS on load
    int lagrange = -1;            // round 1 commits the wires from their VALUES over the Lagrange-basis key derived from the SRS (same proof
                                  // bytes): -1 = from 2^18 gates on (below, the heavy-bucket paths of small scalars cost more than they save: 2^15 gates 3.93 against 3.73 ms) when a sample of the witness
                                  // shows small values (a dense witness gains nothing from the key), --lagrange = always,
                                  // --no-lagrange = never (from the masked coefficient forms, as the reference does)
};

template <class C>
int run(bool ultra, uint64_t num_gates, int reps, int range_bits, const Options& opt, const char* circuit_file = nullptr) {
    using Fr = Fp64<typename C::Fr>;
    if (opt.gpus == 1) check(mzk_init(-1), "mzk_init");                  // (with several devices each worker thread binds its own)
    auto t0 = std::chrono::steady_clock::now();
    BenchCircuitHost<C> host = circuit_file ? BenchCircuitHost<C>::read(circuit_file) : BenchCircuitHost<C>::generate(num_gates, ultra, range_bits, !opt.device_preprocess);
    ultra = host.ultra;
    if (std::getenv("MZK_PROVE_CORRUPT_WITNESS"))                       // test hook: wire 0 of row 5 takes the value of row 6 -> gate 5 no longer holds
    {
        host.wires[5] = host.wires[6];
        if (!host.witness.empty()) host.witness[host.wire_variables[5]] = host.witness[host.wire_variables[6]];
    }
    ChaChaRng rng = test_rng();
    const Fr beta = fr_rand<typename C::Fr>(rng);                       // the SRS trapdoor: first draw of the bench's rng (bench.rs:50-54)
    const auto beta_c = canonical(beta);                                // (drawn with --srs too, then unused: the same blinders follow)
    const SrsFile srs_file = opt.srs_path ? SrsFile::read(opt.srs_path, C::ID) : SrsFile();
    ShardedProver<C> sp(opt.gpus);
    sp.transcript = opt.transcript;
    double circuit_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    const bool lagrange = opt.lagrange < 0 ? (host.log_n >= 18 && host.witness_is_small()) : opt.lagrange != 0;
    const KeyFile key_file = opt.pk_path ? KeyFile::read(opt.pk_path, (opt.pk_uncompressed ? 0u : MZK_SER_COMPRESSED) | (opt.pk_check ? MZK_KEY_CHECK_COMMITMENTS : 0u)) : KeyFile();
    sp.setup(host, beta_c, opt.host_witness, lagrange, opt.slice_srs, opt.srs_path ? &srs_file : nullptr, opt.device_preprocess, opt.pk_path ? &key_file : nullptr);    // SRS, circuit upload and PlonkKzgSnark::preprocess on every device
    const double preprocess_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    size_t pk_bytes = key_file.bytes.size();
    if (opt.save_pk_path) {
        if (opt.gpus > 1 && opt.slice_srs) throw std::runtime_error("--save-pk: with --gpus G every rank holds a slice of the commit key; add --no-slice");
        const std::vector<uint8_t> image = sp.prover[0]->serialize_key(!opt.pk_uncompressed, host.pub_input.size());
        FILE* fp = std::fopen(opt.save_pk_path, "wb");
        if (!fp || std::fwrite(image.data(), 1, image.size(), fp) != image.size()) throw std::runtime_error(std::string("--save-pk: cannot write ") + opt.save_pk_path);
        std::fclose(fp);
        pk_bytes = image.size();
    }
    if (opt.derive_variables) sp.derive_wire_variables();
    if (opt.check_witness) {
        const mzk_witness_report rep = sp.check_witness();
        const unsigned long long n = 1ull << host.log_n;
        if (rep.kind == MZK_CHECK_SATISFIED) std::printf("witness: satisfied");
        else if (rep.kind == MZK_CHECK_GATE) {
            Fr res;
            std::memcpy(res.l, rep.gate_residual, 32);
            const auto v = canonical(res);
            std::printf("witness: gate row %llu residual 0x%016llx%016llx%016llx%016llx", (unsigned long long)rep.gate_row, (unsigned long long)v[3],
                        (unsigned long long)v[2], (unsigned long long)v[1], (unsigned long long)v[0]);
        } else if (rep.kind == MZK_CHECK_LOOKUP) std::printf("witness: lookup row %llu", (unsigned long long)rep.lookup_row);
        else std::printf("witness: copy cell (%llu,%llu) != (%llu,%llu)", (unsigned long long)(rep.copy_cell / n), (unsigned long long)(rep.copy_cell % n),
                         (unsigned long long)(rep.copy_rep_cell / n), (unsigned long long)(rep.copy_rep_cell % n));
        std::printf("; failing gate rows %llu, lookup rows %llu, copy cells %llu%s", (unsigned long long)rep.gate_failures, (unsigned long long)rep.lookup_failures,
                    (unsigned long long)rep.copy_failures, rep.copy_checked ? "" : " (copy constraints not checked: no wire-variable table)");
        if (opt.derive_variables && rep.copy_failures && rep.kind != MZK_CHECK_COPY)
            std::printf("; first copy cell (%llu,%llu) != (%llu,%llu)", (unsigned long long)(rep.copy_cell / n), (unsigned long long)(rep.copy_cell % n),
                        (unsigned long long)(rep.copy_rep_cell / n), (unsigned long long)(rep.copy_rep_cell % n));
        std::printf("\n");
        std::fflush(stdout);
        if (rep.kind != MZK_CHECK_SATISFIED) return 3;
    }
    Proof<C> proof = sp.prove(rng, false, opt.check_agree);             // the proof whose bytes are printed (and warm-up)
    const std::vector<uint8_t> bytes = proof.serialize_compressed();
    double ms = 0, median_ms = 0, min_ms = 0, max_ms = 0;
    if (reps > 0) {
        for (int i = 0; i < 2; i++) sp.prove(rng);
        sp.sync();
        // prove() returns the finished proof, so every repetition can be read off the clock on its own: the mean is what the figures of
        // rounds 1-5 are; the median says what a proof takes when nothing else happens on the host (one in a few dozen takes milliseconds longer)
        std::vector<double> each;
        t0 = std::chrono::steady_clock::now();
        auto t1 = t0;
        for (int i = 0; i < reps; i++) {
            sp.prove(rng);
            const auto t2 = std::chrono::steady_clock::now();
            each.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
            t1 = t2;
        }
        sp.sync();
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
        std::sort(each.begin(), each.end());
        median_ms = each[each.size() / 2]; min_ms = each.front(); max_ms = each.back();
        sp.prove(rng, true);
    }
    Prover<C>& prover = *sp.prover[0];
    std::string hex;
    static const char* d = "0123456789abcdef";
    for (uint8_t b : bytes) { hex.push_back(d[b >> 4]); hex.push_back(d[b & 15]); }
    std::printf("{\"curve\": %d, \"plonk_type\": \"%s\", \"num_gates\": %llu, \"log_n\": %d, \"gpus\": %d, \"host_witness\": %s, \"lagrange_round1\": %s, \"proof_bytes\": %zu, "
                "\"prove_ms\": %.3f, \"prove_median_ms\": %.3f, \"prove_min_ms\": %.3f, \"prove_max_ms\": %.3f, \"circuit_build_s\": %.3f, \"preprocess_s\": %.3f, \"lagrange_key_s\": %.3f, \"rounds_ms\": {",
                C::ID, ultra ? "UltraPlonk" : "TurboPlonk", (unsigned long long)num_gates, host.log_n, opt.gpus, opt.host_witness == 0 ? "false" : (opt.host_witness == 1 ? "\"wire table\"" : "\"witness vector\""), lagrange ? "true" : "false",
                bytes.size(), ms, median_ms, min_ms, max_ms, circuit_s, preprocess_s, sp.lagrange_key_s);
    bool first = true;
    for (auto& kv : prover.timings_ms) { std::printf("%s\"%s\": %.3f", first ? "" : ", ", kv.first.c_str(), kv.second); first = false; }
    std::vector<uint8_t> vk_bytes;                                      // VerifyingKey commitments (selectors, then sigmas), compressed
    for (const auto* v : {&prover.selector_comms, &prover.sigma_comms})
        for (const auto& cm : *v) { uint8_t b[48]; Encoding<C>::g1_bytes(cm, b); vk_bytes.insert(vk_bytes.end(), b, b + C::G1_BYTES); }
    std::string vk_hex;
    for (uint8_t b : vk_bytes) { vk_hex.push_back(d[b >> 4]); vk_hex.push_back(d[b & 15]); }
    std::printf("}, \"pk_bytes\": %zu, \"vk_hex\": \"%s\", \"proof_hex\": \"%s\"}\n", pk_bytes, vk_hex.c_str(), hex.c_str());
    return 0;
}

// --slots K: K proofs in flight on ONE key.  Every thread draws from its own rng with the bench's seed, so that proof i of every slot is
// proof i of the single-slot run made first on the original prover.
template <class C>
int run_slots(bool ultra, uint64_t num_gates, int reps, int range_bits, const Options& opt) {
    using Fr = Fp64<typename C::Fr>;
    using P = Prover<C>;
    check(mzk_init(-1), "mzk_init");
    int32_t device = 0;
    check(mzk_get_device(&device), "mzk_get_device");
    const BenchCircuit<C> cs = BenchCircuit<C>::generate(num_gates, ultra, range_bits);
    const Fr beta = [&] { ChaChaRng r = test_rng(); return fr_rand<typename C::Fr>(r); }();
    const auto beta_c = canonical(beta);
    uint64_t srs = 0;
    check(mzk_srs_generate_for_testing(C::ID, beta_c.data(), cs.n + 3, &srs), "mzk_srs_generate_for_testing");
    const int K = opt.slots, count = std::max(reps, 1);
    std::vector<std::unique_ptr<P>> slots;
    slots.push_back(std::make_unique<P>(srs, cs));
    for (int i = 1; i < K; i++) slots.push_back(slots[i % 2 ? 0 : i - 1]->fork());           // forks of the prover and forks of forks: all peers
    std::vector<P*> family;
    for (auto& s : slots) family.push_back(s.get());
    const typename P::Hbm hbm = slots[0]->hbm();
    const uint64_t family_bytes = P::family_hbm_bytes(family);
    // `count` proofs on one slot; the first call of each pass is warm-up and not timed
    auto pass = [&](P& p, std::vector<std::vector<uint8_t>>& out) {
        ChaChaRng rng = test_rng();
        (void)fr_rand<typename C::Fr>(rng);                                 // the trapdoor's draw (bench.rs:50-54): the blinders follow it
        for (int i = 0; i < count; i++) out.push_back(p.prove(rng, cs, false, opt.transcript).serialize_compressed());
    };
    std::vector<std::vector<uint8_t>> alone, warm;
    pass(*slots[0], warm);
    auto t0 = std::chrono::steady_clock::now();
    pass(*slots[0], alone);
    const double alone_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 1; i < K; i++) { ChaChaRng rng = test_rng(); (void)slots[i]->prove(rng, cs, false, opt.transcript); }                          // warm-up of the other slots
    std::vector<std::vector<std::vector<uint8_t>>> got(K);
    std::vector<std::exception_ptr> errors(K);
    std::vector<std::thread> threads;
    t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < K; i++)
        threads.emplace_back([&, i] {
            try {
                check(mzk_set_device(device), "mzk_set_device");
                pass(*slots[i], got[i]);
            } catch (...) { errors[i] = std::current_exception(); }
        });
    for (auto& t : threads) t.join();
    const double slots_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (auto& e : errors) if (e) std::rethrow_exception(e);
    bool agree = true;
    for (int i = 0; i < K; i++) agree = agree && got[i] == alone;
    std::printf("{\"curve\": %d, \"plonk_type\": \"%s\", \"num_gates\": %llu, \"log_n\": %d, \"slots\": %d, \"proofs_per_slot\": %d, \"proofs_per_s\": %.3f, "
                "\"one_slot_proofs_per_s\": %.3f, \"hbm_fixed_bytes\": %llu, \"hbm_proving_key_bytes\": %llu, \"hbm_workspace_bytes\": %llu, \"hbm_shared_bytes\": %llu, "
                "\"sharers\": %u, \"family_hbm_bytes\": %llu",
                C::ID, ultra ? "UltraPlonk" : "TurboPlonk", (unsigned long long)num_gates, cs.log_n, K, count, (double)K * count / slots_s, count / alone_s,
                (unsigned long long)hbm.fixed, (unsigned long long)hbm.proving_key, (unsigned long long)hbm.workspace, (unsigned long long)hbm.shared, hbm.sharers,
                (unsigned long long)family_bytes);
    if (opt.check_agree) std::printf(", \"slots_agree_with_one_slot\": %s", agree ? "true" : "false");
    std::printf(", \"proof_hex\": \"%s\"}\n", [&] { std::string h; static const char* d = "0123456789abcdef"; for (uint8_t b : alone[0]) { h.push_back(d[b >> 4]); h.push_back(d[b & 15]); } return h; }().c_str());
    std::fflush(stdout);
    slots.clear();
    (void)mzk_srs_release(srs);
    return opt.check_agree && !agree ? 1 : 0;
}

static std::string to_hex(const std::vector<uint8_t>& bytes) {
    std::string hex;
    static const char* d = "0123456789abcdef";
    for (uint8_t b : bytes) { hex.push_back(d[b >> 4]); hex.push_back(d[b & 15]); }
    return hex;
}

template <class C>
int run_link(uint64_t gates1, uint64_t gates2, const GroupLayout& layout, int reps, TranscriptKind transcript) {
    using Fr = Fp64<typename C::Fr>;
    check(mzk_init(-1), "mzk_init");
    BenchCircuit<C> cs1 = BenchCircuit<C>::generate(gates1, false, 8), cs2 = BenchCircuit<C>::generate(gates2, false, 8);
    if (cs1.n != cs2.n) throw std::runtime_error("the two bench circuits must share one domain size");
    ChaChaRng rng = test_rng();
    const Fr beta = fr_rand<typename C::Fr>(rng);
    const auto beta_c = canonical(beta);
    uint64_t srs = 0;
    check(mzk_srs_generate_for_testing(C::ID, beta_c.data(), cs1.n + 3, &srs), "mzk_srs_generate_for_testing");
    Prover<C> p1(srs, cs1), p2(srs, cs2);
    Proof<C> proof1 = p1.prove(rng, cs1, false, transcript);
    LinkingHint<C> h1 = link_hint(p1, proof1);
    Proof<C> proof2 = p2.prove(rng, cs2, false, transcript);
    LinkingHint<C> h2 = link_hint(p2, proof2);
    LinkingProof<C> link = link_proofs<C>(srs, h1, h2, layout, transcript);
    double ms = 0;
    if (reps > 0) {
        check(mzk_dev_sync(), "sync");
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; i++) link_proofs<C>(srs, h1, h2, layout, transcript);
        check(mzk_dev_sync(), "sync");
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    }
    std::printf("{\"curve\": %d, \"log_n\": %d, \"link_ms\": %.3f, \"proof1_hex\": \"%s\", \"proof2_hex\": \"%s\", \"link_proof_hex\": \"%s\"}\n", C::ID, cs1.log_n, ms,
                to_hex(proof1.serialize_compressed()).c_str(), to_hex(proof2.serialize_compressed()).c_str(), to_hex(link.serialize_compressed()).c_str());
    (void)mzk_srs_release(srs);
    return 0;
}

template <class C>
int run_batch(bool ultra, int range_bits, const std::vector<uint64_t>& gates, TranscriptKind transcript) {
    using Fr = Fp64<typename C::Fr>;
    check(mzk_init(-1), "mzk_init");
    std::vector<BenchCircuit<C>> circuits;
    for (uint64_t g : gates) circuits.push_back(BenchCircuit<C>::generate(g, ultra, range_bits));
    ChaChaRng rng = test_rng();
    const Fr beta = fr_rand<typename C::Fr>(rng);
    const auto beta_c = canonical(beta);
    uint64_t srs = 0;
    check(mzk_srs_generate_for_testing(C::ID, beta_c.data(), circuits[0].n + 3, &srs), "mzk_srs_generate_for_testing");
    std::vector<std::unique_ptr<Prover<C>>> owned;
    std::vector<Prover<C>*> provers;
    std::vector<const BenchCircuit<C>*> cs;
    for (auto& c : circuits) {
        if (c.n != circuits[0].n) throw std::runtime_error("circuit domain size != expected domain size");
        owned.push_back(std::make_unique<Prover<C>>(srs, c));
        provers.push_back(owned.back().get());
        cs.push_back(&c);
    }
    const BatchProof<C> proof = batch_prove<C>(rng, provers, cs, transcript);
    std::printf("{\"curve\": %d, \"log_n\": %d, \"instances\": %zu, \"batch_proof_hex\": \"%s\"}\n", C::ID, circuits[0].log_n, gates.size(),
                to_hex(proof.serialize_compressed()).c_str());
    owned.clear();
    (void)mzk_srs_release(srs);
    return 0;
}

int main(int argc_in, char** argv_in) {
    // options anywhere on the line; what is left is positional
    Options opt;
    std::vector<char*> args;
    for (int i = 0; i < argc_in; i++) {
        const std::string a = argv_in[i];
        if (a == "--gpus" && i + 1 < argc_in) opt.gpus = std::atoi(argv_in[++i]);
        else if (a == "--host-witness") opt.host_witness = 1;
        else if (a == "--host-witness-vars") opt.host_witness = 2;
        else if (a == "--check-agree") opt.check_agree = true;
        else if (a == "--slots" && i + 1 < argc_in) opt.slots = std::atoi(argv_in[++i]);
        else if (a == "--transcript" && i + 1 < argc_in) {
            try { opt.transcript = transcript_kind(argv_in[++i]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
        }
        else if (a == "--check-witness") opt.check_witness = true;
        else if (a == "--derive-variables") opt.derive_variables = true;
        else if (a == "--device-preprocess") opt.device_preprocess = true;
        else if (a == "--pk" && i + 1 < argc_in) opt.pk_path = argv_in[++i];
        else if (a == "--save-pk" && i + 1 < argc_in) opt.save_pk_path = argv_in[++i];
        else if (a == "--pk-uncompressed") opt.pk_uncompressed = true;
        else if (a == "--pk-check") opt.pk_check = true;
        else if (a == "--lagrange") opt.lagrange = 1;
        else if (a == "--no-lagrange") opt.lagrange = 0;
        else if (a == "--no-slice") opt.slice_srs = false;
        else if (a == "--srs" && i + 1 < argc_in) opt.srs_path = argv_in[++i];
        else args.push_back(argv_in[i]);
    }
    const int argc = (int)args.size();
    char** argv = args.data();
    if (opt.gpus < 1 || opt.gpus > 16) { std::fprintf(stderr, "mzk_prove: --gpus 1..16\n"); return 2; }
    if (argc < 4) { std::fprintf(stderr, "usage: %s <curve 0|1> <turbo|ultra> <num_gates> [reps] [range_bit_len] [--gpus G] [--transcript merlin|solidity] [--host-witness | --host-witness-vars] [--check-agree] [--check-witness] [--derive-variables] [--device-preprocess] [--no-lagrange] [--srs FILE] [--save-pk FILE] [--pk FILE (file)] [--pk-uncompressed] [--pk-check]\n", argv[0]); return 2; }
    const int curve = std::atoi(argv[1]);
    if (opt.device_preprocess && (std::string(argv[2]) == "file" || std::string(argv[2]) == "link" || std::string(argv[2]) == "batch")) {
        std::fprintf(stderr, "mzk_prove: --device-preprocess needs the circuit's variable table: a circuit file holds sigma values, not variables "
                             "(bench circuits only: <turbo|ultra> <num_gates>)\n");
        return 2;
    }
    if (opt.derive_variables && (opt.host_witness == 2 || opt.slots || std::string(argv[2]) == "link" || std::string(argv[2]) == "batch")) {
        std::fprintf(stderr, "mzk_prove: --derive-variables goes with turbo, ultra and file, and not with --host-witness-vars (a witness vector in the circuit's "
                             "numbering) or --slots\n");
        return 2;
    }
    if (opt.pk_path && std::string(argv[2]) != "file") {
        std::fprintf(stderr, "mzk_prove: --pk goes with `file`: the key replaces the circuit file's selector and sigma values, its witness and public input stay\n");
        return 2;
    }
    if ((opt.pk_path || opt.save_pk_path) && (opt.slots || std::string(argv[2]) == "link" || std::string(argv[2]) == "batch")) {
        std::fprintf(stderr, "mzk_prove: --pk / --save-pk go with turbo, ultra and file\n");
        return 2;
    }
    if (std::string(argv[2]) == "link") {
        if (argc < 8) { std::fprintf(stderr, "usage: %s <curve 0|1> link <num_gates_1> <num_gates_2> <alignment> <offset> <size> [reps]\n", argv[0]); return 2; }
        const GroupLayout layout{(uint32_t)std::atoi(argv[5]), std::strtoull(argv[6], nullptr, 10), std::strtoull(argv[7], nullptr, 10)};
        const uint64_t g1 = std::strtoull(argv[3], nullptr, 10), g2 = std::strtoull(argv[4], nullptr, 10);
        const int reps = argc > 8 ? std::atoi(argv[8]) : 0;
        try {
            return curve == 0 ? run_link<Bls12_381>(g1, g2, layout, reps, opt.transcript) : run_link<Bn254>(g1, g2, layout, reps, opt.transcript);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "mzk_prove: %s\n", e.what());
            return 1;
        }
    }
    if (std::string(argv[2]) == "batch") {
        if (argc < 6) { std::fprintf(stderr, "usage: %s <curve 0|1> batch <turbo|ultra> <range_bit_len> <num_gates> ...\n", argv[0]); return 2; }
        std::vector<uint64_t> gates;
        for (int i = 5; i < argc; i++) gates.push_back(std::strtoull(argv[i], nullptr, 10));
        try {
            const bool u = std::string(argv[3]) == "ultra";
            return curve == 0 ? run_batch<Bls12_381>(u, std::atoi(argv[4]), gates, opt.transcript) : run_batch<Bn254>(u, std::atoi(argv[4]), gates, opt.transcript);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "mzk_prove: %s\n", e.what());
            return 1;
        }
    }
    if (std::string(argv[2]) == "file") {
        try {
            const int reps = argc > 4 ? std::atoi(argv[4]) : 0;
            return curve == 0 ? run<Bls12_381>(false, 0, reps, 8, opt, argv[3]) : run<Bn254>(false, 0, reps, 8, opt, argv[3]);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "mzk_prove: %s\n", e.what());
            return 1;
        }
    }
    const bool ultra = std::string(argv[2]) == "ultra";
    const uint64_t gates = std::strtoull(argv[3], nullptr, 10);
    const int reps = argc > 4 ? std::atoi(argv[4]) : 0, range_bits = argc > 5 ? std::atoi(argv[5]) : 8;
    if (opt.slots) {
        if (opt.slots < 1 || opt.slots > 16 || opt.gpus != 1) { std::fprintf(stderr, "mzk_prove: --slots 1..16, on one device (a sharded prover cannot be forked)\n"); return 2; }
        try {
            return curve == 0 ? run_slots<Bls12_381>(ultra, gates, reps, range_bits, opt) : run_slots<Bn254>(ultra, gates, reps, range_bits, opt);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "mzk_prove: %s\n", e.what());
            return 1;
        }
    }
    try {
        return curve == 0 ? run<Bls12_381>(ultra, gates, reps, range_bits, opt) : run<Bn254>(ultra, gates, reps, range_bits, opt);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mzk_prove: %s\n", e.what());
        return 1;
    }
}
