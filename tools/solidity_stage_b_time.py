"""Stage B (Fiat-Shamir) of the batch verifier alone, K single BN254 TurboPlonk proofs, under the Merlin and the Keccak-256 (Solidity)
transcript in ONE process on one card: HIP-event time of the library's profile region "vfy_transcript" (warm-up, then the mean and the
spread of `reps` launches each), next to the number of Keccak-f[1600] permutations either transcript costs per proof (counted on the
host transcripts, which absorb what the kernels absorb).  Prints the text of profiles/solidity_transcript_time.txt.

    python tools/solidity_stage_b_time.py [K] [reps]
"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import mpc_jellyfish_amd as mj
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    L = lib.init(0)
    c = mj.params.BN254
    cs = mj.snark.gen_circuit_for_bench(c, 20, "TurboPlonk")
    rng = mj.rng.test_rng()
    beta = mj.rng.fr_rand(c, rng)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)
    _, h, beta_h = mj.kzg.open_key_for_testing(c, beta)
    vk = mj.keys.VerifyingKey.deserialize(c.curve_id, pk.serialize_vk(0, h, beta_h))
    # permutations per proof, counted where the host transcripts call the permutation / hash
    T = mj.transcript
    counts, proofs = {}, {}
    real_f, real_sq = T.keccak_f1600, T.SolidityTranscript.get_and_append_challenge
    n_perm = [0]

    def counted_f(state):
        n_perm[0] += 1
        real_f(state)

    def counted_sq(self, label):
        n = 64 + len(self.transcript)                              # absorbed once up to the last full block, the tail finished twice
        n_perm[0] += n // 136 + 2 * (2 if n % 136 == 135 else 1)
        return real_sq(self, label)

    T.keccak_f1600, T.SolidityTranscript.get_and_append_challenge = counted_f, counted_sq
    for kind in ("merlin", "solidity"):
        pk.__dict__.pop("_transcript_heads", None)
        n_perm[0] = 0
        _, proofs[kind] = mj.snark.prove(mj.rng.test_rng(), cs, pk, transcript=kind)
        counts[kind] = n_perm[0]                                   # (Merlin: STROBE's initial permutation included, as the kernel runs it)
    T.keccak_f1600, T.SolidityTranscript.get_and_append_challenge = real_f, real_sq
    v = vk.verifier()
    times = {}
    lib.check(L.mzk_profile_enable(1), "mzk_profile_enable")
    for kind in ("merlin", "solidity"):
        assert mj.snark.verify(vk, [], proofs[kind], None, transcript=kind)
        batch = [proofs[kind]] * K
        for _ in range(3):
            v.begin(batch, [[]] * K, transcript=kind).discard()
        samples = []
        for _ in range(reps):
            lib.check(L.mzk_profile_reset(), "mzk_profile_reset")
            v.begin(batch, [[]] * K, transcript=kind).discard()
            ms, cnt = lib.profile_get("vfy_transcript")
            assert cnt == 1
            samples.append(ms)
        times[kind] = samples
    lib.check(L.mzk_profile_enable(0), "mzk_profile_enable")
    m = {k: statistics.mean(s) for k, s in times.items()}
    print("Stage B (Fiat-Shamir) of mzk_verifier_batch_begin alone under the two transcripts: MI355X, one card, one process.")
    print("K = %d single TurboPlonk proofs on BN254 (bench circuit of 20 gates, n = 2^%d, no public input, compressed), one proof image repeated;" % (K, cs.n.bit_length() - 1))
    print("HIP events around the one kernel (profile region vfy_transcript), 3 warm-up launches, then %d launches each." % reps)
    print()
    for kind in ("merlin", "solidity"):
        s = times[kind]
        print("  %-9s mean %8.3f ms   min %8.3f   max %8.3f   stdev %6.3f   Keccak-f[1600] permutations per proof: %d" %
              (kind, m[kind], min(s), max(s), statistics.pstdev(s), counts[kind]))
    print()
    print("  time ratio solidity / merlin         %.2f" % (m["solidity"] / m["merlin"]))
    print("  permutation ratio solidity / merlin  %.2f" % (counts["solidity"] / counts["merlin"]))
    vk.release_verifier()
    pk.release()
    ck.release()


if __name__ == "__main__":
    main()
