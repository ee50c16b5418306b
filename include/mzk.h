/* mzk.h -- C ABI of libmi355zk: the MI355X (gfx950) backend for the jf-plonk prover's
 * arithmetic hot path (radix-2 NTT over Fr, Pippenger MSM on G1).
 *
 * The reference (renegade-fi/mpc-jellyfish) has no FFI of its own: the path sits behind two
 * third-party Rust trait surfaces.  Each entry point below names the reference call it replaces
 * (paths relative to the reference tree); INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   curve_id        0 = BLS12-381, 1 = BN254.
 *   field elements  little-endian 64-bit limbs; Fr = 4 limbs; Fq = 6 limbs (BLS12-381) / 4 (BN254).
 *                   "mont" = Montgomery form a*R mod p with R = 2^(64*limbs), fully reduced --
 *                   the in-memory image of ark-ff's Fp<MontBackend<_,N>,N>.
 *   affine points   packed x||y (mont), no flag word; (0,0) encodes the point at infinity.
 *   Jacobian out    X||Y||Z (mont); Z = 0 encodes infinity (ark-ec `Projective::new_unchecked(X,Y,Z)`).
 *   return value    0 on success, < 0 on error (mzk_strerror); never unwinds, never aborts.
 *   threading       every entry point may be called concurrently (the reference calls commit and
 *                   fft from Rayon workers: univariate_kzg/mod.rs:125-127, prover.rs:552-562);
 *                   the kernels of all calls ON ONE DEVICE are enqueued under that device's lock (its
 *                   plan cache and workspace), but the host-pointer entry points move their operands on
 *                   per-call I/O streams outside it, so one caller's transfers overlap another's
 *                   kernels (see mzk_host_alloc).  Calls on different devices never contend (mzk_init).
 *   memory          host buffers are borrowed for the duration of the call; the library owns all
 *                   device memory it allocates, including the registered SRS copy.
 *   "_dev" variants take device pointers (hipMalloc / torch tensors) and a hipStream_t passed as
 *                   void* (NULL = the null stream); they do not synchronise unless stated.
 */
#ifndef MZK_H
#define MZK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MZK_API __attribute__((visibility("default")))
#else
#define MZK_API
#endif

#define MZK_OK 0
#define MZK_ERR_INVALID_ARG (-1)
#define MZK_ERR_HIP (-2)          /* a HIP runtime call failed; text via mzk_last_error() */
#define MZK_ERR_NO_DEVICE (-3)
#define MZK_ERR_BAD_HANDLE (-4)
#define MZK_ERR_UNSUPPORTED (-5)
#define MZK_ERR_OOM (-6)
#define MZK_ERR_NOT_INIT (-7)
#define MZK_ERR_LOOKUP (-8)       /* Plookup: a lookup value is not in the table (constraint_system.rs:1410-1412) */

#define MZK_CURVE_BLS12_381 0
#define MZK_CURVE_BN254 1

/* Create the library's context on HIP device `device` if it has none yet and bind the CALLING THREAD to it (idempotent;
 * -1 = the thread's / the process's current binding, else the current HIP device).  Fails with MZK_ERR_NO_DEVICE when no GPU
 * is visible: there is no CPU fallback.
 *
 * Several devices from one process (`mzk_init(n_devices)`, "copies to device(s) once"; 8(e)): call
 * mzk_init(g) for every device g, one host thread per device.  Each device has its own context -- lock, workspace, NTT plan
 * cache, I/O slots, SRS and proving-key registries -- so calls on different devices run concurrently and share nothing.
 * SRS and proving-key handles carry their device: a call that takes one runs on that device whatever thread makes it.  Calls
 * that take bare device pointers (mzk_ntt_dev, mzk_poly_*, mzk_dev_*, the register functions) run on the calling thread's
 * device: the last mzk_init / mzk_set_device on that thread, or -- for threads that never bound one, e.g. the Rayon workers of a
 * single-GPU prover -- the first device initialised.  Device memory belongs to the device it was allocated on; between devices
 * it moves with mzk_dev_copy_peer.
 * MZK_VIRTUAL_DEVICES=G (environment, read at mzk_init): devices 0..G-1 exist whatever the machine has, mapped round-robin onto
 * the physical GPUs -- G full contexts on one card, to rehearse a multi-GPU host on a one-GPU box (results are identical). */
MZK_API int32_t mzk_init(int32_t device);
/* Rebind the calling thread to an initialised device / report its binding / number of devices mzk_init accepts. */
MZK_API int32_t mzk_set_device(int32_t device);
MZK_API int32_t mzk_get_device(int32_t* out_device);
MZK_API int32_t mzk_device_count(int32_t* out_count);
/* Releases every context (all devices). */
MZK_API int32_t mzk_shutdown(void);
MZK_API const char* mzk_strerror(int32_t code);
MZK_API const char* mzk_last_error(void);
MZK_API const char* mzk_version(void);

/* ---- SRS (CommitKey = UnivariateProverParam{powers_of_g}; primitives/src/pcs/univariate_kzg/srs.rs:36-40) ---- */

/* Copy n_points affine bases to the device once; returns an opaque handle. */
MZK_API int32_t mzk_srs_register(int32_t curve_id, const uint64_t* xy_mont, uint64_t n_points, uint64_t* out_handle);
MZK_API int32_t mzk_srs_register_dev(int32_t curve_id, const void* d_xy_mont, uint64_t n_points, uint64_t* out_handle, void* stream);
MZK_API int32_t mzk_srs_release(uint64_t handle);
/* Testing SRS on the device: point i = beta^i * G (G = standard generator), beta canonical 4 limbs.
 * Mirrors gen_srs_for_testing (srs.rs:118-153) with g fixed to the generator. */
MZK_API int32_t mzk_srs_generate_for_testing(int32_t curve_id, const uint64_t* beta_canonical, uint64_t n_points, uint64_t* out_handle);
/* The same with a base point of the caller's: point i = beta^i * g, g affine x||y (mont), on the curve and in the subgroup (not
 * checked).  `universal_setup_for_testing` (plonk/src/proof_system/snark.rs:495-517) draws beta = Fr::rand, then g = G1::rand and
 * h = G2::rand from the same rng: a host that mirrors those draws passes its g here.  g_xy_mont = NULL: the standard generator. */
MZK_API int32_t mzk_srs_generate_for_testing_g(int32_t curve_id, const uint64_t* beta_canonical, const uint64_t* g_xy_mont, uint64_t n_points,
                                               uint64_t* out_handle);
/* The testing SRS over the LAGRANGE basis of the gate domain H (|H| = 2^log_n, generated by the primitive root w): point i = L_i(beta) g
 * for i < 2^log_n, then n_extra points beta^j (beta^n - 1) g = the commitments of X^j Z_H(X).  For a polynomial p with values v_i = p(w^i)
 * and its masked form p + (b_0 + b_1 X + ..) Z_H (mask_polynomial, prover.rs:463-486), an MSM of (v_0 .. v_(n-1), b_0, b_1, ..) over this
 * SRS is the SAME group element as the commitment of the masked coefficients over beta^i g (univariate_kzg/mod.rs:90-116) -- but the
 * scalars are the witness VALUES, which are mostly small numbers (flags, counters, 64-bit amounts): their high digits are zero and the MSM
 * touches a fraction of the table rows (mzk_msm_*: zero digits cost nothing, heavy buckets have their own kernels).  Round 1 of both
 * hosts commits the wires this way when given such a key.  (From an SRS without trapdoor the same points are the inverse group-NTT of
 * its first 2^log_n points: mzk_srs_lagrange_from_srs.) */
MZK_API int32_t mzk_srs_generate_lagrange_for_testing(int32_t curve_id, const uint64_t* beta_canonical, const uint64_t* g_xy_mont, uint32_t log_n,
                                                      uint32_t n_extra, uint64_t* out_handle);
/* The same key from the points of a registered SRS alone (no trapdoor): [L_i(beta)]g = (1/n) sum_j w^(-ij) [beta^j]g, the inverse NTT over the
 * group of its first 2^log_n points, then [beta^(n+j)]g - [beta^j]g for the n_extra tail (the SRS must hold 2^log_n + n_extra points).
 * (n / 2) log2 n scalar multiplications: 0.51 s at 2^20 on BLS12-381, 0.22 s on BN254 -- once per SRS and domain size.  Set-up peak:
 * (5n + 8) internal points of scratch (1.17 GB at 2^20 on BLS12-381), handed back before the call returns.  Synchronises. */
MZK_API int32_t mzk_srs_lagrange_from_srs(uint64_t srs_handle, uint32_t log_n, uint32_t n_extra, uint64_t* out_handle);
/* A new SRS handle holding the points [first, first + n_points) of a registered one (a device copy; `trim` generalised, srs.rs:77-93): a rank
 * of a multi-GPU prover keeps the range it commits over -- 1 / G of the points and of the fixed-base table, built with the window that suits
 * the slice's size -- and hands it to mzk_prover_create as its commit key (see there).  The source stays registered. */
MZK_API int32_t mzk_srs_slice(uint64_t handle, uint64_t first, uint64_t n_points, uint64_t* out_handle);
MZK_API int32_t mzk_srs_download(uint64_t handle, uint64_t first, uint64_t n_points, uint64_t* out_xy_mont);
/* ---- serialized SRS: the G1 records of ark-serialize 0.4 (CanonicalSerialize of UnivariateProverParam / UnivariateUniversalParams)
 * Records only: the container (u64 LE count, the trailing G2 elements h and beta_h) belongs to the caller.  Sizes and flags:
 *   BLS12-381  compressed 48 B: x big-endian; byte 0: 0x80 compressed (must be set), 0x40 infinity, 0x20 y is the larger
 *              uncompressed 96 B: x BE || y BE; byte 0: 0x80 and 0x20 must be clear, 0x40 infinity
 *   BN254      compressed 32 B: x little-endian; byte 31: 0x80 y is the larger, 0x40 infinity, both set = invalid
 *              uncompressed 64 B: x LE (no flags) || y LE with those flags in byte 63 (0x80 written as ark writes it, ignored on read)
 * ("y is the larger": y > q - y on canonical integers.)  Checks, as ark's deserialize_* (MZK_SER_VALIDATE) / deserialize_*_unchecked:
 * always the flag rules, x, y < q, and for compressed records that x^3 + b is a square; MZK_SER_VALIDATE adds on-curve for uncompressed
 * records and, on BLS12-381, membership in G1 (the endomorphism test phi(P) = -[u^2]P, equivalent to [r]P = O).
 * UNLIKE ark, a point at infinity is always refused (MZK_ERR_ENCODING): the affine SRS has no usable infinity -- (0, 0) would corrupt the
 * mixed additions of an MSM -- and a KZG power at infinity means beta = 0.  So is an uncompressed (0, 0) read without validation.
 * On MZK_ERR_ENCODING *out_bad_index (nullable) is the lowest failing index and mzk_last_error() reads "point <i>: <reason>", the first
 * check that point failed in the order flags, range, square / on-curve, subgroup, infinity; otherwise *out_bad_index = UINT64_MAX.
 * On any failure no handle exists and nothing stays allocated.  One thread per point decodes (csrc/srs_io.hip), then the internal table
 * is built as by mzk_srs_register; threading and device binding are those of mzk_srs_register[_dev].  n_points = 0 is valid.
 * The host variant stages the records whole: one copy, one decode (profile regions srs_load.copy / .decode / .table). */
#define MZK_SER_COMPRESSED 1u
#define MZK_SER_VALIDATE 2u
MZK_API int32_t mzk_srs_register_serialized(int32_t curve_id, const uint8_t* point_bytes, uint64_t n_points, uint32_t flags, uint64_t* out_handle,
                                            uint64_t* out_bad_index);
/* The same from device memory (any alignment), read on `stream`; synchronises it. */
MZK_API int32_t mzk_srs_register_serialized_dev(int32_t curve_id, const void* d_point_bytes, uint64_t n_points, uint32_t flags, uint64_t* out_handle,
                                                uint64_t* out_bad_index, void* stream);
/* Points [first, first + n_points) of any SRS handle as records (flags: MZK_SER_COMPRESSED or 0) into out_bytes (host,
 * n_points * record bytes); (0, 0) is written as ark writes infinity.  Synchronises. */
MZK_API int32_t mzk_srs_serialize(uint64_t handle, uint64_t first, uint64_t n_points, uint32_t flags, uint8_t* out_bytes);

MZK_API int32_t mzk_srs_len(uint64_t handle, uint64_t* out_n_points);

/* ---- serialized ProvingKey / VerifyingKey: the CanonicalSerialize image of jf-plonk's keys (ark-serialize 0.4, derive order;
 * DESIGN.md section 4.13).  The image names neither its curve nor its mode: the caller states both, as for the SRS; the mode
 * (MZK_SER_COMPRESSED or not) applies to every point in it.
 *   usize            u64 little-endian
 *   bool             1 byte, 0 or 1 (anything else is invalid);  Option<T>: a bool, then T if it is 1;  Vec<T>: u64 LE count, then the items
 *   Fr               32 B little-endian, the canonical integer, no flag bits, below r (both curves)
 *   DensePolynomial  its coeffs: Vec<Fr> (from_coefficients_vec strips trailing zeros: shorter than n is normal, the zero polynomial has
 *                    count 0; trailing zero coefficients are accepted, as ark accepts them)
 *   Commitment       its G1Affine: records and flags as for the serialized SRS above
 *   G2               opaque bytes, neither decoded nor validated: BLS12-381 96 / 192 B, BN254 64 / 128 B (compressed / uncompressed)
 *   ProvingKey    (plonk/src/proof_system/structs.rs:575-590)
 *     sigmas: Vec<Poly>  selectors: Vec<Poly>  commit_key: Vec<G1>  vk: VerifyingKey  plookup_pk: Option<PlookupProvingKey>
 *   PlookupProvingKey (:595-607)  range_table_poly, key_table_poly, table_dom_sep_poly, q_dom_sep_poly (4 Poly)
 *   VerifyingKey  (:682-707)
 *     domain_size: usize  num_inputs: usize  sigma_comms: Vec<G1>  selector_comms: Vec<G1>  k: Vec<Fr>
 *     open_key: { g: G1, h: G2, beta_h: G2 } (primitives/src/pcs/univariate_kzg/srs.rs:48-55)  is_merged: bool  plookup_vk: Option<4 x G1> (:771-785)
 * Parity of this restatement with the Rust code is UNPINNED until tests/golden/ref_proving_keys.json (integration/rust gen_fixtures,
 * family proving_key) exists: the tests build their images from the format as written here.
 *
 * mzk_key_layout: host-only (no GPU, no mzk_init), reads nothing outside [bytes, bytes + len), and of the image only length prefixes
 * and tags.  flags: MZK_SER_COMPRESSED (the mode) and MZK_KEY_VK_ONLY (the image is a bare VerifyingKey: the polynomial, commit-key and
 * has_plookup fields stay zero, vk_off = 0); other bits are ignored.  Offsets are byte offsets into the image; those of a Vec point at
 * its first item, past the count.  MZK_ERR_ENCODING, with mzk_last_error() naming the field and the reason: "truncated in <field> at
 * byte <len>" (every count is compared with the bytes left divided by the record size, so a count of 2^64 - 1 is truncated, never a
 * wrapped product); a bool or Option tag that is not 0 or 1; a sigma count that is not 5 or 6; a selector count that is not 13 (W = 5) /
 * 14 (W = 6); plookup_pk present when W is not 6 or absent when it is; plookup_pk and plookup_vk not both present or absent;
 * sigma_comms / selector_comms / k counts that do not match W and nsel; domain_size no power of two or above 2^27; a polynomial with
 * more than domain_size coefficients; fewer than domain_size + 3 commit-key points; bytes left over after the last field. */
#define MZK_KEY_CHECK_COMMITMENTS 4u   /* mzk_prover_create_serialized: the commitments of vk must commit the polynomials of the key */
#define MZK_KEY_VK_ONLY 8u             /* mzk_key_layout: a bare VerifyingKey image */
typedef struct mzk_key_layout {
    uint32_t num_wire_types, num_selectors;             /* W = 5 or 6, nsel = 13 or 14 */
    uint32_t has_plookup, has_plookup_vk, is_merged, reserved;
    uint64_t domain_size, num_inputs;
    uint64_t g1_record_bytes, g2_record_bytes;          /* of the stated curve and mode */
    uint64_t sigma_off[6], sigma_len[6];                /* per polynomial: offset of its first coefficient, coefficient count */
    uint64_t selector_off[14], selector_len[14];
    uint64_t table_off[4], table_len[4];                /* range, key, table_dom_sep, q_dom_sep */
    uint64_t commit_key_off, commit_key_count;
    uint64_t vk_off, vk_len;                            /* the embedded VerifyingKey as a whole */
    uint64_t sigma_comms_off, selector_comms_off, k_off, g_off, h_off, beta_h_off, plookup_comms_off;
    uint64_t total_len;
} mzk_key_layout_t;
MZK_API int32_t mzk_key_layout(int32_t curve_id, const uint8_t* bytes, uint64_t len, uint32_t flags, mzk_key_layout_t* out);

/* Fr records on the device (csrc/key_io.cuh), the primitives of the key loader as mzk_srs_register_serialized_dev's decode is of the
 * SRS loader.  mzk_fr_decode_dev: ONE launch for up to 32 segments of one staged image (device, image_len bytes; its base 4-byte
 * aligned, as any allocation is; the records at any byte alignment): segment s holds
 * counts[s] records of 32 B from byte src_offsets[s] of d_image on and fills row dst_rows[s] < n_rows of d_out (n_rows rows of row_len aligned
 * Montgomery elements): slot i < counts[s] is the record, checked to be below r and converted; slots counts[s] <= i < row_len are zero.
 * counts[s] <= row_len < 2^40, every segment inside the image (MZK_ERR_INVALID_ARG otherwise, nothing is launched).  A record not below r: MZK_ERR_ENCODING, *out_bad_segment / *out_bad_index (nullable; UINT32_MAX / UINT64_MAX when
 * all is well) the LOWEST (segment, index) in segment order -- one atomicMin on a 64-bit word, the same answer on every run -- and
 * mzk_last_error() "segment <s> coefficient <i>: not below the modulus"; the rows are then unspecified.  Synchronises `stream`.
 * mzk_fr_encode_dev: count aligned Montgomery elements at d_in -> count records of 32 B at d_out (device, 4-byte aligned).  Asynchronous. */
MZK_API int32_t mzk_fr_decode_dev(int32_t curve_id, const void* d_image, uint64_t image_len, uint32_t n_segments, const uint64_t* src_offsets,
                                  const uint64_t* counts, const uint32_t* dst_rows, void* d_out, uint32_t n_rows, uint64_t row_len,
                                  uint32_t* out_bad_segment, uint64_t* out_bad_index, void* stream);
MZK_API int32_t mzk_fr_encode_dev(int32_t curve_id, const void* d_in, uint64_t count, void* d_out, void* stream);

/* ---- host pairing (csrc/hostpairing.hpp): G2 and the optimal ate pairing of both curves, for the verifier's final
 * check multi_pairing([A, -B], [beta_h, h]) == 1 (plonk/src/proof_system/verifier.rs:226-250) and for the G2 half of an OpenKey.
 * Every entry point of this block is host-only like mzk_key_layout: no GPU, no mzk_init, nothing kept between calls.
 *
 * G2 records (ark-serialize 0.4; Fq2 = c0 + c1 u; "y is the larger" = y > -y with c1 compared first, then c0, on canonical integers):
 *   BLS12-381  compressed    96 B  x.c1 || x.c0, each 48 B big-endian; byte 0: 0x80 compressed (must be set), 0x40 infinity, 0x20 y is the larger
 *              uncompressed 192 B  x.c1 || x.c0 || y.c1 || y.c0; byte 0: 0x80 and 0x20 must be clear, 0x40 infinity
 *   BN254      compressed    64 B  x.c0 || x.c1, each 32 B little-endian; last byte: 0x80 y is the larger, 0x40 infinity, both = invalid
 *              uncompressed 128 B  x.c0 || x.c1 || y.c0 || y.c1; the same flags in the last byte (written; 0x80 ignored on read)
 * mzk_g2_decode: one record (flags: MZK_SER_COMPRESSED states its mode) -> out_xy_mont = x.c0, x.c1, y.c0, y.c1, Montgomery Fq (4 x 6 resp.
 * 4 x 4 limbs).  The checks of mzk_srs_register_serialized in its order -- flag bits, infinity (always refused: an OpenKey has none), every
 * coordinate below q, x^3 + b' a square in Fq2 (compressed) or, with MZK_SER_VALIDATE, on the twist (uncompressed) -- and with
 * MZK_SER_VALIDATE [r]Q = O on BOTH curves (BN254's twist has a cofactor too).  MZK_ERR_ENCODING: mzk_last_error() = "G2: <reason>", the
 * reasons those of the G1 decoder.
 * mzk_g2_mul: [k]Q as a record of the same mode, k a canonical integer of 4 limbs (any value below 2^256), Q = q_bytes decoded as above
 * or, NULL, the standard generator; [k]Q = O is written as the infinity record.  beta_h = [beta]h of a testing OpenKey (srs.rs:118-153).
 * mzk_pairing_product_is_one: *out = 1 when prod_{i<n} e(P_i, Q_i) = 1, else 0: n Miller loops, ONE final exponentiation.  g1_xy_mont: n x
 * (x, y) Montgomery Fq, the boundary form of every G1 point of this ABI, (0, 0) = infinity (contributes 1); g2_xy_mont: n x the output of
 * mzk_g2_decode.  n = 0: 1.  The points are taken as members of G1 and G2 (what mzk_g2_decode checks under MZK_SER_VALIDATE); nothing is
 * checked here.
 * mzk_pairing_gt: e(P, Q) as 12 canonical Fq integers (12 x 6 resp. 12 x 4 limbs), the coefficients of 1, w, .., w^11 in
 * Fq[w] / (w^12 - 2 xi0 w^6 + xi0^2 + 1), xi0 = 1 (BLS12-381) / 9 (BN254): the tower's w with u = w^6 - xi0, the representation of
 * oracle/pyref_pairing.ExtField.  The value is f_{ate,Q}(P)^((q^12 - 1) / r) with the Miller value conjugated for BLS12-381's negative x, as
 * ark-ec does: on BN254 it EQUALS pyref_pairing's PairingCurve.pairing(Q, P), on BLS12-381 it is that value's INVERSE (pyref_pairing ignores
 * the sign of x).  Products compared with 1 do not see the difference.
 * mzk_batch_verify_challenge: r of batch_verify_opening_proofs (verifier.rs:203-215) from the K challenges u of the proofs (Montgomery Fr,
 * caller's order): 1 for K = 1; else a Merlin transcript "batch verify", K appends of u under "u" (32 B little-endian), 64 challenge
 * bytes under "r" reduced mod r (csrc/merlin.cuh, the transcript code of the device compiled for the host).  K = 0: MZK_ERR_INVALID_ARG.
 * mzk_batch_verify_challenge_t: the same r under the transcript kind that `flags` names -- 0: mzk_batch_verify_challenge; 
 * MZK_TRANSCRIPT_SOLIDITY: 1 for K = 1, else one challenge of a SolidityTranscript (below) whose transcript is the K values u as 32 B
 * little-endian canonical and whose state is zero.  Any other bit, K = 0: MZK_ERR_INVALID_ARG. */
MZK_API int32_t mzk_g2_decode(int32_t curve_id, const uint8_t* bytes, uint32_t flags, uint64_t* out_xy_mont);
MZK_API int32_t mzk_g2_mul(int32_t curve_id, const uint8_t* q_bytes, const uint64_t* k_canonical, uint32_t flags, uint8_t* out_bytes);
MZK_API int32_t mzk_pairing_product_is_one(int32_t curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, uint64_t n, int32_t* out);
MZK_API int32_t mzk_pairing_gt(int32_t curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, uint64_t* out);
MZK_API int32_t mzk_batch_verify_challenge(int32_t curve_id, const uint64_t* u_mont, uint64_t K, uint64_t* out_r_mont);
MZK_API int32_t mzk_batch_verify_challenge_t(int32_t curve_id, uint32_t flags, const uint64_t* u_mont, uint64_t K, uint64_t* out_r_mont);

/* ---- the Keccak-256 transcript: SolidityTranscript (plonk/src/transcript/solidity.rs:31-78; csrc/keccak_transcript.cuh, one code for host and
 * device), the transcript of proofs that an EVM-style keccak256 verifier checks.  The label of new() and of every append is dropped;
 * `transcript` is the concatenation of the appended messages (the ark-serialize compressed bytes the Merlin transcript takes), `state` 64
 * bytes, zero at first.  get_and_append_challenge: state = keccak256(state || transcript || 0x00) || keccak256(state || transcript || 0x01),
 * challenge = state[0..48] little-endian mod r; the transcript is NOT cleared and the challenge is NOT appended, so every challenge hashes
 * the whole transcript so far behind the new state.  An empty extra message therefore equals none.  keccak256 is sha3::Keccak256: rate 136,
 * pad byte 0x01 (not SHA3's 0x06).
 * MZK_TRANSCRIPT_SOLIDITY in `flags` of mzk_verifier_batch_begin, mzk_verifier_aggregate_begin and mzk_verifier_link_begin: the device's
 * Fiat-Shamir stage runs this transcript instead of Merlin, over the same messages in the same order (one thread per proof, the transcript in
 * a slot of device memory sized from the key's shape and the longest extra message; the two digests of a challenge share one absorption).
 * Without the flag nothing changes; with challenges_mont / eta_mont given the flag has no effect.  One batch_verify uses one kind
 * throughout: r comes from mzk_batch_verify_challenge_t with the same flag.
 * Host-only (no GPU, no mzk_init), for hosts that write such proofs outside Rust:
 * mzk_keccak256: out32 = keccak256(msg[0..len]) ("the quick brown fox jumps over the lazy dog" -> 865bf05c..14ec; "" -> c5d24601..a470).
 * mzk_solidity_challenge: ONE get_and_append_challenge -- state64 (in, out: 64 zero bytes before the first challenge), the WHOLE transcript so
 * far (len bytes, nullable when len = 0); *out_mont the challenge, Montgomery Fr. */
#define MZK_TRANSCRIPT_SOLIDITY 4u
MZK_API int32_t mzk_keccak256(const uint8_t* msg, uint64_t len, uint8_t* out32);
MZK_API int32_t mzk_solidity_challenge(int32_t curve_id, uint8_t* state64, const uint8_t* transcript, uint64_t len, uint64_t* out_mont);

/* ---- verifier: PlonkKzgSnark::batch_verify / verify (snark.rs:141-190, 653-671; verifier.rs:68-251) for single-instance `Proof`s of
 * TurboPlonk and UltraPlonk (csrc/verifier.cuh).  K >= 1 proofs under ONE verifying key go through the device in one
 * pass -- per proof 13 | 18 G1 decodings, one Merlin transcript, the linearisation scalars -- and end in two MSMs; groups under different
 * keys with the same open key are summed before ONE check of two pairings (host).  verify is K = 1 with r = 1.  Needs mzk_init.
 *
 * mzk_verifier_create: a bare VerifyingKey image (mzk_key_layout with MZK_KEY_VK_ONLY; flags: MZK_SER_COMPRESSED states the mode of the key
 * AND of every proof verified under it, MZK_SER_VALIDATE adds the subgroup checks to the key's points).  is_merged: MZK_ERR_UNSUPPORTED.
 * Kept on the device: the decoded commitments (selectors, sigmas, Ultra: the 4 Plookup commitments, open_key.g), k, and the byte script of
 * append_vk_and_pub_input (transcript/mod.rs:45-104); h and beta_h are decoded on the host.  A key commitment at infinity is normal (an
 * unused selector commits to nothing): it is flagged, not refused.  MZK_ERR_ENCODING: "vk.<field>: <reason>".
 * mzk_verifier_shape: points per proof (13 | 18), bases of the key (nsel + W + 4 (Ultra) + 1), the length of a proof image under this key
 * and mode, num_inputs (each nullable).
 *
 * A batch runs in two phases, because r depends on every proof's u.
 * mzk_verifier_batch_begin: K images of proof_len bytes each, back to back; public_inputs_canonical: K x num_inputs canonical integers of 4
 * limbs; extra_ranges (nullable: no proof has an extra transcript message): K pairs (begin, end) of byte offsets into extra_msgs, begin =
 * UINT64_MAX for a proof without one; challenges_mont (nullable): K x 7 Montgomery Fr (tau, beta, gamma, alpha, zeta, v, u) that REPLACE
 * the transcript -- for callers with another transcript (Rescue); flags: MZK_SER_VALIDATE (subgroup checks of the proofs' points),
 * MZK_TRANSCRIPT_SOLIDITY (the Keccak-256 transcript instead of Merlin, above).  On the host: proof_len, the Vec counts and the Option tag against the key's type.  On the device: A decode, B Fiat-Shamir, C
 * scalars (one per base: repeated bases are summed).  *out_u_mont (nullable): the K challenges u, for mzk_batch_verify_challenge.
 * Any malformed proof: MZK_ERR_ENCODING, *out_bad_index (nullable) the LOWEST bad proof -- one 64-bit atomicMin, the same answer on every
 * run -- and mzk_last_error() "proof <i>: <field>: <reason>": a bad length, count or tag, a point (reasons of mzk_srs_register_serialized;
 * infinity is flagged, not refused), an evaluation or public input "not below the modulus".  No batch is left open then.
 * mzk_verifier_batch_challenges: K x 7 Montgomery Fr.  mzk_verifier_batch_scalars (each nullable): K x NKEY scalars for the key's bases
 * (selectors, sigmas, Ultra: range, key, table_dom_sep, q_dom_sep; open_key.g last and zero: its scalar is the finish's), K x NP for the proof's
 * own points in image order (wires, prod_perm, split_quot, opening = zeta, shifted_opening = u zeta w, Ultra: h_1, h_2, prod_lookup), K
 * aggregated evaluations; Montgomery Fr, unweighted.
 * mzk_verifier_batch_finish: weights proof i by r_weights_mont[i] (r^i of mzk_batch_verify_challenge, in the caller's order across groups),
 * column-sums the key rows and the evaluations by a fixed tree (no atomics on field elements), zeroes the scalar of every flagged base and runs
 * the two MSMs of verifier.rs:217-247 through the variable-base path: A = sum r^i (W_i + u_i W'_i), B over the key's bases, the K x NP proof
 * points and -(sum r^i eval_i) g; Jacobian (x, y, z) Montgomery Fq.  The batch handle is consumed, also on failure; with all three pointers
 * NULL the batch is only discarded.
 * mzk_verifier_check: sums n_groups results (same open key), normalises, *out_accept = [ e(A, beta_h) e(-B, h) == 1 ].
 *
 * Handles and threads.  A verifier lives on the device of the thread that created it (MZK_ERR_NOT_INIT without one) and its handle, like
 * the handle of every batch begun under it, carries that device: any thread may call with them whatever device it is bound to, and finds
 * its own binding unchanged on return.  mzk_verifier_destroy refuses a verifier that has an open batch (MZK_ERR_INVALID_ARG, "the verifier
 * has an open batch"; the verifier stays usable).  A destroy that races a call in flight on another thread is safe: the handle is gone at
 * once, the call completes on the object it found, and the memory is freed when that call returns.  mzk_shutdown releases every verifier
 * and open batch; their handles are MZK_ERR_BAD_HANDLE afterwards. */
MZK_API int32_t mzk_verifier_create(int32_t curve_id, const uint8_t* vk_bytes, uint64_t len, uint32_t flags, uint64_t* out_handle);
MZK_API int32_t mzk_verifier_destroy(uint64_t verifier);
MZK_API int32_t mzk_verifier_shape(uint64_t verifier, uint32_t* out_n_proof_points, uint32_t* out_n_key_bases, uint64_t* out_proof_len, uint64_t* out_num_inputs);
MZK_API int32_t mzk_verifier_batch_begin(uint64_t verifier, const uint8_t* proofs, uint64_t proof_len, uint64_t K, const uint64_t* public_inputs_canonical,
                                         const uint8_t* extra_msgs, const uint64_t* extra_ranges, const uint64_t* challenges_mont, uint32_t flags,
                                         uint64_t* out_batch, uint64_t* out_u_mont, uint64_t* out_bad_index);
MZK_API int32_t mzk_verifier_batch_challenges(uint64_t batch, uint64_t* out);
MZK_API int32_t mzk_verifier_batch_scalars(uint64_t batch, uint64_t* out_key_rows, uint64_t* out_proof_rows, uint64_t* out_evals);
MZK_API int32_t mzk_verifier_batch_finish(uint64_t batch, const uint64_t* r_weights_mont, uint64_t* out_A_xyz, uint64_t* out_B_xyz);
MZK_API int32_t mzk_verifier_check(uint64_t verifier, const uint64_t* A_xyz, const uint64_t* B_xyz, uint64_t n_groups, int32_t* out_accept);

/* ---- aggregated proofs: PlonkKzgSnark::verify_batch_proof (snark.rs:117-138; verifier.rs:68-184, 256-321) for `BatchProof`s of m >= 1
 * instances under a TUPLE of m verifiers ("Aggregated proofs").  K BatchProofs under one tuple go through the device in
 * one pass and leave an ordinary batch handle: mzk_verifier_batch_challenges / _scalars / _finish (discard too) and mzk_verifier_check take
 * it as they take a single-proof batch, so the (A, B) of aggregated and of single-proof groups with one open key sum into one check.
 *
 * A BatchProof image (ark-serialize, derive order; structs.rs:266-291), every Vec a u64 count and its items:
 *   wires_poly_comms_vec: Vec<Vec<G1>> (m x W)   prod_perm_poly_comms_vec: Vec<G1> (m)
 *   poly_evals_vec: Vec<{ wires_evals: Vec<Fr> (W), wire_sigma_evals: Vec<Fr> (W - 1), perm_next_eval: Fr }> (m)
 *   plookup_proofs_vec: Vec<Option<{ h_poly_comms: Vec<G1> (2), prod_lookup_poly_comm: G1, 15 Fr }>> (m)
 *   split_quot_poly_comms: Vec<G1> (W)   opening_proof: G1   shifted_opening_proof: G1
 * mzk_batch_proof_layout: host-only like mzk_key_layout (no GPU, no mzk_init).  The length of an image of m instances of one type (ultra: 0 |
 * 1) on this curve and in this mode (flags: MZK_SER_COMPRESSED) and the offset of every record; offsets of a Vec point at its first item.
 * With `image` (nullable) the container of that image of `len` bytes is checked as mzk_verifier_aggregate_begin checks it before anything is
 * staged -- the length, every Vec count and every Option tag, in image order -- MZK_ERR_ENCODING with mzk_last_error() "instance <j>: <field>:
 * <reason>", j = m for what belongs to the whole proof (the length, the outer counts, split_quot_poly_comms).  m = 0: MZK_ERR_INVALID_ARG;
 * m > MZK_VERIFIER_MAX_INSTANCES: MZK_ERR_UNSUPPORTED.
 *
 * The tuple: every verifier of the same curve, device, image mode, domain size, open key (MZK_ERR_INVALID_ARG otherwise: "the verification
 * keys have different open keys", "the domain size of the <j>-th verification key is different", ..) and Plonk type (a mixed tuple:
 * MZK_ERR_UNSUPPORTED -- batch_prove makes no such proof).  One handle may stand at several positions (a key and its forks); everything is
 * laid out per POSITION.
 * mzk_verifier_aggregate_shape (host-only): points per BatchProof NP(m) = m (W + 1) + W + 2 + 3 m ultra; key bases NKEY(m) = m (NKEY_1 - 1)
 * + 1; the image length; the public inputs per proof, sum_j num_inputs_j (each nullable).
 * mzk_verifier_aggregate_begin: the contract of mzk_verifier_batch_begin with K BatchProof images and, per proof, the m instances' public
 * inputs back to back in tuple order.  Column order, which mzk_verifier_batch_scalars reports and the MSM B follows:
 *   key columns    position 0's block (selectors, sigmas, Ultra: range, key, table_dom_sep, q_dom_sep), position 1's, .., open_key.g last
 *   proof columns  j < m: wires_j (W), prod_perm_j; then split_quot (W), opening, shifted_opening; then, Ultra, j < m: h_1, h_2, prod_lookup
 * (m = 1: exactly the single-proof orders).  Any malformed proof: MZK_ERR_ENCODING, *out_bad_index the LOWEST bad proof and mzk_last_error()
 * "proof <i>: instance <j>: <field>: <reason>" -- the lowest proof, then its lowest instance, then its first field, on every run (one 64-bit
 * atomicMin over proof << 40 | instance << 33 | field << 4 | reason); no batch is left open.  An open aggregate batch holds every verifier
 * of its tuple: mzk_verifier_destroy of any of them is refused until the batch is finished or discarded. */
#define MZK_VERIFIER_MAX_INSTANCES 64u
typedef struct mzk_batch_proof_layout {
    uint32_t m, num_wire_types, ultra, g1_record_bytes;
    uint64_t total_len;
    uint64_t wires_off[MZK_VERIFIER_MAX_INSTANCES], prod_perm_off[MZK_VERIFIER_MAX_INSTANCES];          /* instance j: its W wire commitments; its permutation product */
    uint64_t wires_evals_off[MZK_VERIFIER_MAX_INSTANCES], sigma_evals_off[MZK_VERIFIER_MAX_INSTANCES], perm_next_off[MZK_VERIFIER_MAX_INSTANCES];
    uint64_t plookup_tag_off[MZK_VERIFIER_MAX_INSTANCES];                                               /* the Option tag; the next three: Ultra only, else 0 */
    uint64_t h_off[MZK_VERIFIER_MAX_INSTANCES], prod_lookup_off[MZK_VERIFIER_MAX_INSTANCES], plookup_evals_off[MZK_VERIFIER_MAX_INSTANCES];
    uint64_t split_quot_off, opening_off, shifted_opening_off;
} mzk_batch_proof_layout_t;
MZK_API int32_t mzk_batch_proof_layout(int32_t curve_id, uint32_t ultra, uint32_t m, uint32_t flags, const uint8_t* image, uint64_t len,
                                       mzk_batch_proof_layout_t* out);
MZK_API int32_t mzk_verifier_aggregate_shape(const uint64_t* verifiers, uint32_t m, uint32_t* out_n_proof_points, uint32_t* out_n_key_bases,
                                             uint64_t* out_proof_len, uint64_t* out_num_inputs);
MZK_API int32_t mzk_verifier_aggregate_begin(const uint64_t* verifiers, uint32_t m, const uint8_t* proofs, uint64_t proof_len, uint64_t K,
                                             const uint64_t* public_inputs_canonical, const uint8_t* extra_msgs, const uint64_t* extra_ranges,
                                             const uint64_t* challenges_mont, uint32_t flags, uint64_t* out_batch, uint64_t* out_u_mont,
                                             uint64_t* out_bad_index);

/* ---- proof links: PlonkKzgSnark::verify_link_proof (proof_linking.rs:240-286; DESIGN.md section 4.14, "Proof links").  A link of two proofs
 * over a GroupLayout (relation/src/proof_linking/mod.rs:16-54) is the KZG opening of a_1 - a_2 - Z_D(eta) q at eta with value 0
 * (univariate_kzg/mod.rs:194-216): it ends in the pair A = pi, B = a_1 - a_2 - Z_D(eta) Q + eta pi.  K links go through the device in one
 * pass and leave an ordinary batch handle, so their (A, B) sums with the (A, B) of single-proof and aggregate groups under the same open key
 * into ONE check of two pairings.
 *
 * mzk_verifier_create_open_key: a verifier handle that carries an OpenKey alone -- g (G1), h, beta_h (G2) as records of the mode
 * MZK_SER_COMPRESSED states; MZK_SER_VALIDATE adds the subgroup checks, as in mzk_verifier_create.  MZK_ERR_ENCODING: "open_key.<field>:
 * <reason>".  The handle rules above hold for it (the device of the calling thread, destroy refused with an open batch, released by
 * mzk_shutdown).  mzk_verifier_shape reports 0 points, 0 key bases, length 0, 0 inputs; mzk_verifier_batch_begin and _aggregate_begin (and
 * _aggregate_shape) return MZK_ERR_INVALID_ARG, "the verifier holds no verifying key"; mzk_verifier_check works with it.
 *
 * mzk_verifier_link_begin: `verifier` is ANY verifier handle, a full key or an open key: its curve, device and image mode are used.
 * records: K x 4 G1 records of that mode, per link lhs.wires_poly_comms[0] (PROOF_LINK_WIRE_IDX = 0), rhs.wires_poly_comms[0],
 * quotient_commitment, opening_proof -- the caller cuts the first two out of the two Plonk proof images.  layouts: K x 3 values (alignment,
 * offset, size).  eta_mont (nullable): K Montgomery Fr that REPLACE the transcript stage (the seam of challenges_mont); flags:
 * MZK_SER_VALIDATE (subgroup checks of the records), MZK_TRANSCRIPT_SOLIDITY (eta from the Keccak-256 transcript); *out_eta_mont (nullable): the K challenges.  On the host, before anything is staged:
 * K = 0 and an alignment above the field's two-adicity (32 | 28): MZK_ERR_INVALID_ARG; a size above 2^27, the largest domain of the library:
 * MZK_ERR_UNSUPPORTED; offset + size beyond 2^alignment is accepted -- the roots wrap or repeat, as mzk_poly_div_roots_dev and the
 * reference's loop take them.  On the device: A decode (the decoder of the proofs), Bl the transcript "PlonkLinkingProof" (the two wire
 * commitments under "linking_wire_comms", the quotient commitment under "quotient_comm", eta; commitments in their compressed form), Cl
 * Z_D(eta) = prod_{i < size} (eta - g^(offset + i)), g the 2^alignment-th root of unity of the NTT, one wave per link.  Any malformed record:
 * MZK_ERR_ENCODING, *out_bad_index (nullable) the LOWEST bad link -- one 64-bit atomicMin, the same answer on every run -- and
 * mzk_last_error() "link <i>: <field>: <reason>", the field one of lhs.wires_poly_comms[0] | rhs.wires_poly_comms[0] | quotient_commitment |
 * opening_proof, the reasons those of mzk_srs_register_serialized; no batch is left open then.  Infinity is flagged, not refused: two proofs
 * of one circuit link with Q = pi = O (proof_linking.rs:124-127).
 * The batch: mzk_verifier_batch_scalars, _finish (discard too) and mzk_verifier_check take it under their contracts above with NKEY = 1
 * (open_key.g, scalar zero: the opened value is 0), NP = 4 with the unweighted row (1, -1, -Z_D(eta), eta), evaluation 0 and A = sum w_i
 * pi_i.  mzk_verifier_batch_challenges: MZK_ERR_INVALID_ARG (a link has no seven challenges).
 * mzk_verifier_link_values (each nullable): K x eta_i and K x Z_D(eta_i), Montgomery Fr.
 * mzk_verifier_link_weights: the K weights for mzk_verifier_batch_finish.  K = 1 and r_mont NULL: exactly 1, so one link alone is the
 * reference's check.  Otherwise (host; csrc/merlin.cuh as mzk_batch_verify_challenge uses it) a Merlin transcript "batch verify links":
 * r_mont, when given, under "r" (32 B little-endian canonical), per link in order eta_i under "eta", per link in order the staged
 * opening-proof record as it stands under "opening_proof", 64 challenge bytes under "s" reduced mod r; weight i = s^(i + 1).  This batching
 * is the library's own (the reference verifies links one at a time).  The pi_i enter because eta_i binds a_1, a_2 and Q but not pi_i:
 * weights blind to them would let two opening "proofs" be chosen jointly so that two false links cancel.  No weight is 1, and r -- the
 * challenge of the Plonk groups checked together with the links -- is absorbed, because the first Plonk proof has weight r^0 = 1. */
MZK_API int32_t mzk_verifier_create_open_key(int32_t curve_id, const uint8_t* g_bytes, const uint8_t* h_bytes, const uint8_t* beta_h_bytes, uint32_t flags,
                                             uint64_t* out_handle);
MZK_API int32_t mzk_verifier_link_begin(uint64_t verifier, const uint8_t* records, uint64_t K, const uint64_t* layouts, const uint64_t* eta_mont, uint32_t flags,
                                        uint64_t* out_batch, uint64_t* out_eta_mont, uint64_t* out_bad_index);
MZK_API int32_t mzk_verifier_link_values(uint64_t batch, uint64_t* out_eta_mont, uint64_t* out_vanishing_mont);
MZK_API int32_t mzk_verifier_link_weights(uint64_t batch, const uint64_t* r_mont, uint64_t* out_weights_mont);

/* ---- KZG openings: UnivariateKzgPCS::verify and batch_verify (univariate_kzg/mod.rs:195-271; DESIGN.md section 4.14, "KZG openings").  The
 * opening of a commitment C at the point z to the value v with proof pi holds iff e(C - v g + z pi, h) = e(pi, beta_h): it ends in the pair
 * A = pi, B = C + z pi - v g.  K openings go through the device in one pass and leave an ordinary batch handle, whose (A, B) sums with the
 * (A, B) of proof, aggregate and link groups under the same open key into ONE check of two pairings.
 *
 * mzk_verifier_open_begin: `verifier` is ANY verifier handle, a full key or an open key: its curve, device and image mode are used.
 * records: K x 2 G1 records of that mode, per opening the commitment, then the opening proof.  points_canonical, values_canonical: K x 4
 * limbs each.  flags: MZK_SER_VALIDATE only (subgroup checks of the records).  On the host, before anything is staged: K = 0 and any other
 * flag bit: MZK_ERR_INVALID_ARG.  On the device: A decode (the decoder of the proofs), Co one thread per opening: z and v range-checked
 * against r and brought to Montgomery form.  A malformed opening: MZK_ERR_ENCODING, *out_bad_index (nullable) the LOWEST bad opening -- one
 * 64-bit atomicMin, the same answer on every run -- and mzk_last_error() "opening <i>: <field>: <reason>", the field one of commitment |
 * proof | point | value (the first of them that is bad), the reasons of a record those of mzk_srs_register_serialized, of a scalar "not
 * below the modulus"; no batch is left open then.  Infinity is flagged, not refused: the zero polynomial commits to O, and a constant
 * polynomial opens with pi = O.
 * The batch: mzk_verifier_batch_scalars, _finish (discard too) and mzk_verifier_check take it under their contracts above with NKEY = 1
 * (open_key.g), NP = 2 with the unweighted row (1, z_i), evaluation v_i, A = sum w_i pi_i and B = sum w_i (C_i + z_i pi_i) - (sum w_i v_i) g.
 * mzk_verifier_batch_challenges, mzk_verifier_link_values and mzk_verifier_link_weights: MZK_ERR_INVALID_ARG, the message names the kind.
 * The handle rules above hold (destroy of the verifier refused while the batch is open, released by mzk_shutdown).
 * Weights are the caller's (r_weights_mont of mzk_verifier_batch_finish).  The reference's batch_verify takes w_0 = 1 and a random 128-bit
 * w_i for every further opening; one opening with weight 1 is the reference's verify.  MIXED CHECKS: when an openings group is summed with
 * other groups in one mzk_verifier_check, none of its weights may be 1 -- the first Plonk proof has weight r^0 = 1, and two members of
 * one sum under equal weights can be chosen jointly so that their errors cancel (the reason given for links above). */
MZK_API int32_t mzk_verifier_open_begin(uint64_t verifier, const uint8_t* records, uint64_t K, const uint64_t* points_canonical,
                                        const uint64_t* values_canonical, uint32_t flags, uint64_t* out_batch, uint64_t* out_bad_index);

/* ---- MSM: replaces <E::G1 as VariableBaseMSM>::msm_bigint(bases, bigints)
 *      at univariate_kzg/mod.rs:109-111 (commit) and :151-155 (open).
 * Computes sum_{i<n} scalars[i] * srs[base_offset + i]; base_offset = num_leading_zeros of
 * skip_leading_zeros_and_convert_to_bigints (mod.rs:379-388).  scalars: n x 4 limbs, canonical
 * integers (msm_bigint semantics) or, with scalars_are_mont != 0, Montgomery Fr as stored in a
 * DensePolynomial (saves the CPU-side into_bigint pass, mod.rs:390-395).
 * n = 0 yields infinity.  Fails with MZK_ERR_INVALID_ARG if base_offset + n exceeds the SRS
 * (the reference's degree guard, mod.rs:98-104).
 * The result POINT is unique; its Jacobian representative (X, Y, Z) is not (bucket entries are ordered by atomics),
 * exactly as ark-ec's Projective result is only defined up to scaling: normalise before comparing or hashing, as the
 * reference does with `.into_affine()` (mod.rs:111) -- mzk_msm_affine / mzk_g1_jacobian_to_affine. */
MZK_API int32_t mzk_msm(uint64_t srs_handle, uint64_t base_offset, const uint64_t* scalars, uint64_t n,
                int32_t scalars_are_mont, uint64_t* out_xyz_mont);
/* Device-resident scalars; the result lands in host memory (the call synchronises the stream). */
MZK_API int32_t mzk_msm_dev(uint64_t srs_handle, uint64_t base_offset, const void* d_scalars, uint64_t n,
                    int32_t scalars_are_mont, uint64_t* out_xyz_mont, void* stream);
/* batch_commit (mod.rs:119-131) in one call: n_polys independent MSMs over one SRS. */
MZK_API int32_t mzk_msm_batch(uint64_t srs_handle, uint32_t n_polys, const uint64_t* const* scalars, const uint64_t* lens,
                      const uint64_t* base_offsets, int32_t scalars_are_mont, uint64_t* out_xyz_mont);
/* Device-resident scalars: d_scalars[i] is a device pointer to lens[i] x 4 limbs.  The MSMs run back to back
 * and share one bucket-reduction phase and one host synchronisation; base_offsets may be NULL (all 0). */
MZK_API int32_t mzk_msm_batch_dev(uint64_t srs_handle, uint32_t n_polys, const void* const* d_scalars, const uint64_t* lens,
                          const uint64_t* base_offsets, int32_t scalars_are_mont, uint64_t* out_xyz_mont, void* stream);
/* Same point as mzk_msm but normalised on the host: x||y (mont), (0,0) for infinity
 * (the `.into_affine()` of mod.rs:111 folded in). */
MZK_API int32_t mzk_msm_affine(uint64_t srs_handle, uint64_t base_offset, const uint64_t* scalars, uint64_t n,
                       int32_t scalars_are_mont, uint64_t* out_xy_mont);

/* Host-only (no GPU needed): out = sum of n Jacobian points (X||Y||Z mont each).  Used to combine the
 * per-GPU partial sums of a point-range-sharded MSM after an all-gather; RCCL has
 * no EC-add reduction, so the "all-reduce of partial EC sums" is all-gather + this local sum. */
MZK_API int32_t mzk_g1_sum_jacobian(int32_t curve_id, const uint64_t* xyz_mont, uint64_t n, uint64_t* out_xyz_mont);

/* Host-only: n Jacobian points -> affine x||y ((0,0) for infinity): `.into_affine()` (mod.rs:111) / normalize_batch. */
MZK_API int32_t mzk_g1_jacobian_to_affine(int32_t curve_id, const uint64_t* xyz_mont, uint64_t n, uint64_t* out_xy_mont);

/* Host-only: the Keccak-f[1600] permutation on 200 bytes (lane (x, y) at byte offset 8 (x + 5 y), little-endian): the
 * primitive under merlin's STROBE-128, for hosts that mirror the transcript of plonk/src/transcript/standard.rs:16-46
 * outside Rust (the Python prover mirror; a Rust caller keeps using merlin). */
MZK_API int32_t mzk_keccak_f1600(uint8_t* state200);

/* Host-only: n_blocks consecutive 64-byte ChaCha blocks (djb variant: 64-bit block counter in state words 12-13, stream id 0) as
 * 16 little-endian u32 words each -- rand_chacha's ChaCha{8,12,20}Rng core, for hosts that mirror `jf_utils::test_rng()`
 * (utilities/src/lib.rs:62-70: the blinders of mask_polynomial / split_quotient_polynomial) and
 * `compute_coset_representatives` (relation/src/constants.rs:30-80) outside Rust. */
MZK_API int32_t mzk_chacha_blocks(const uint32_t key[8], uint64_t counter, uint32_t rounds, uint32_t n_blocks, uint32_t* out_words);

/* ---- NTT: replaces EvaluationDomain::{fft,ifft}_in_place on Radix2EvaluationDomain
 *      forward coset: plonk/src/proof_system/prover.rs:554,557,561,566,567,579-591
 *      inverse coset: plonk/src/proof_system/prover.rs:672
 *      inverse plain: relation/src/constraint_system.rs:1172,1189,1221,1240,1257,1266-1287,1366,1414-1415
 * data: 2^log_n x 4 limbs (mont), transformed in place, natural order in and out.  Elements at
 * index >= in_len are treated as zero on input (the reference zero-pads short coefficient
 * vectors).  coset_offset_mont = NULL means offset 1; otherwise one Fr (mont), e.g. Fr::GENERATOR
 * for `quot_domain.get_coset(Fr::GENERATOR)` (prover.rs:545).
 *   forward: out[i] = sum_j c[j] (h w^i)^j      inverse: c[j] = h^-j N^-1 sum_i e[i] w^(-ij) */
MZK_API int32_t mzk_ntt(int32_t curve_id, uint64_t* data_mont, uint64_t in_len, uint32_t log_n, int32_t inverse,
                const uint64_t* coset_offset_mont);
MZK_API int32_t mzk_ntt_batch(int32_t curve_id, uint32_t n_polys, uint64_t* const* data_mont, const uint64_t* in_lens,
                      uint32_t log_n, int32_t inverse, const uint64_t* coset_offset_mont);
/* Device-resident: `batch` polynomials of 2^log_n elements each, `batch_stride` elements apart
 * (>= 2^log_n), transformed in place.  in_len applies to every polynomial.  coset_offset_mont is
 * a HOST pointer.  Asynchronous on `stream`. */
MZK_API int32_t mzk_ntt_dev(int32_t curve_id, void* d_data_mont, uint64_t in_len, uint32_t log_n, int32_t inverse,
                    const uint64_t* coset_offset_mont, uint32_t batch, uint64_t batch_stride, void* stream);

/* ---- TurboPlonk quotient round on the device: replaces the body of
 *      Prover::compute_quotient_polynomial, plonk/src/proof_system/prover.rs:512-673 (one instance, no Plookup).
 * mzk_plonk_pk_register keeps, per proving key, the coset evaluations of the 13 selector and 5 sigma
 * polynomials (`ProvingKey{selectors, sigmas}`, plonk/src/proof_system/structs.rs:575-590) on the
 * 8n-point quotient domain -- the reference recomputes those 18 FFTs in every proof (prover.rs:552-558).
 * selector_coeffs: 13 x poly_len, sigma_coeffs: 5 x poly_len Montgomery coefficients (low order first,
 * selector order q_lc[4], q_mul[2], q_hash[4], q_o, q_c, q_ecc); k_mont: the 5 coset representatives
 * `vk.k` (relation/src/constants.rs:30-80). */
MZK_API int32_t mzk_plonk_pk_register(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const uint64_t* selector_coeffs,
                                      const uint64_t* sigma_coeffs, uint64_t poly_len, const uint64_t* k_mont, uint64_t* out_handle);
MZK_API int32_t mzk_plonk_pk_release(uint64_t pk_handle);
/* d_polys: device buffer of (5 + 2) x 8n elements: wire polynomials, then the permutation product z,
 * then the public-input polynomial, each as coefficients in its first in_len slots (the rest is
 * ignored).  The buffer is overwritten with the coset evaluations.  alpha/beta/gamma: host, Montgomery.
 * d_out: 8n elements, the coefficients of the quotient polynomial (what `coset.ifft` returns at
 * prover.rs:672; the caller strips trailing zeros as DensePolynomial::from_coefficients_vec does).
 * Asynchronous on `stream`. */
MZK_API int32_t mzk_plonk_quotient_dev(uint64_t pk_handle, void* d_polys, uint64_t in_len, const uint64_t* alpha_mont,
                                       const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_out, void* stream);
/* Host-pointer form: polys = 7 x in_len coefficients (wires, z, pi), out = 8n coefficients. */
MZK_API int32_t mzk_plonk_quotient(uint64_t pk_handle, const uint64_t* polys, uint64_t in_len, const uint64_t* alpha_mont,
                                   const uint64_t* beta_mont, const uint64_t* gamma_mont, uint64_t* out);

/* ---- UltraPlonk (Plookup).  The proving key additionally holds q_lookup as the 14th
 * selector, a 6th wire type (sigma, k) and the four table polynomials `PlookupProvingKey{range_table_poly,
 * key_table_poly, table_dom_sep_poly, q_dom_sep_poly}` (plonk/src/proof_system/structs.rs:592-640).
 * selector_coeffs: 14 x poly_len, sigma_coeffs: 6 x poly_len, table_coeffs: 4 x poly_len in the order range, key,
 * table_dom_sep, q_dom_sep; k_mont: 6 coset representatives. */
MZK_API int32_t mzk_plonk_pk_register_ultra(int32_t curve_id, uint32_t log_n, const uint64_t* selector_coeffs, const uint64_t* sigma_coeffs,
                                            const uint64_t* table_coeffs, uint64_t poly_len, const uint64_t* k_mont, uint64_t* out_handle);
/* Quotient with the Plookup terms (prover.rs:512-673 with compute_quotient_plookup_contribution, :773-888).
 * d_polys: (6 + 2 + 3) x 8n elements: wires, z, public input, h_1, h_2, Plookup product polynomial. */
MZK_API int32_t mzk_plonk_quotient_ultra_dev(uint64_t pk_handle, void* d_polys, uint64_t in_len, const uint64_t* tau_mont,
                                             const uint64_t* alpha_mont, const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_out,
                                             void* stream);
/* Round 1.5: replaces compute_merged_lookup_table (relation/src/constraint_system.rs:1290-1309) and the merge of
 * compute_lookup_sorted_vec_polynomials (:1370-1417, before its two iFFTs).  d_wire_values: 6 x n wire evaluations.
 * Outputs (device): merged table (n), merged lookup witness (n), sorted vector (2n - 1): h_1 = ifft(sorted[..n]),
 * h_2 = ifft(sorted[n-1..]).  Returns MZK_ERR_LOOKUP when a looked-up value is not in the table.  Synchronises. */
MZK_API int32_t mzk_plookup_sorted_vec_dev(uint64_t pk_handle, const void* d_wire_values, const uint64_t* tau_mont, void* d_merged_table,
                                           void* d_merged_lookup, void* d_sorted, void* stream);
/* Round 2.5: replaces compute_lookup_prod_polynomial (constraint_system.rs:1311-1368; one division per row there).
 * d_out: the n coefficients of the (unmasked) Plookup product polynomial.  Asynchronous. */
MZK_API int32_t mzk_plookup_product_dev(uint64_t pk_handle, const void* d_merged_table, const void* d_merged_lookup, const void* d_sorted,
                                        const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_out, void* stream);

/* ---- Coset-chunked quotient for multi-GPU proving.  The 8n-point coset g*H_8n is the union of the 8
 * cosets h_k*H_n, h_k = g*w_8n^k (the residue classes of the point index mod 8); the closure of prover.rs:605-659 reads
 * index i and (i + 8) mod 8n only, so each class is self-contained.  A chunked key holds the fixed polynomials on the listed
 * classes only (strictly increasing `classes`, each < 8); num_wire_types 5 (table_coeffs NULL) or 6.
 * mzk_plonk_quotient_chunked_dev: d_polys = (W + 2 [+ 3]) rows of in_stride elements, coefficients in the first in_len
 * (<= 2n) slots, NOT overwritten; d_out = n_classes x n elements: for each resident class k the n coefficients of
 * t mod (X^n - h_k^n) (local inverse coset NTT done).  After the ranks exchange these (one all-gather / all-to-all),
 * mzk_plonk_quotient_combine_dev turns the 8 class remainders (class-major, 8 x n) into the 8n coefficients that
 * `coset.ifft` returns at prover.rs:672 (an 8-point inverse DFT per coefficient index). */
MZK_API int32_t mzk_plonk_pk_register_chunked(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const uint64_t* selector_coeffs,
                                              const uint64_t* sigma_coeffs, const uint64_t* table_coeffs, uint64_t poly_len,
                                              const uint64_t* k_mont, const uint32_t* classes, uint32_t n_classes, uint64_t* out_handle);
MZK_API int32_t mzk_plonk_quotient_chunked_dev(uint64_t pk_handle, const void* d_polys, uint64_t in_stride, uint64_t in_len,
                                               const uint64_t* tau_mont, const uint64_t* alpha_mont, const uint64_t* beta_mont,
                                               const uint64_t* gamma_mont, void* d_out, void* stream);
/* The same with flags.  MZK_QUOTIENT_PI_ZERO: the caller's public-input polynomial (row W + 1 of d_polys) is the zero polynomial -- a circuit
 * without public inputs, or all of them zero: its row is then neither transformed nor read (one coset NTT in W + 2 less per class). */
#define MZK_QUOTIENT_PI_ZERO 1u
MZK_API int32_t mzk_plonk_quotient_chunked_flags_dev(uint64_t pk_handle, const void* d_polys, uint64_t in_stride, uint64_t in_len, uint32_t flags,
                                                     const uint64_t* tau_mont, const uint64_t* alpha_mont, const uint64_t* beta_mont,
                                                     const uint64_t* gamma_mont, void* d_out, void* stream);
MZK_API int32_t mzk_plonk_quotient_combine_dev(int32_t curve_id, uint32_t log_n, const void* d_class_remainders, void* d_out, void* stream);
/* The same recovery from FEWER classes.  The quotient has degree W (n + 1) + 2 (`quotient_polynomial_degree`,
 * plonk/src/proof_system/prover.rs:916-919, 1126-1128), below (W + 1) n once n > W + 2: the remainders modulo X^n - h_k^n on any
 * W + 1 classes -- 6 of the 8 for TurboPlonk, 7 for UltraPlonk -- determine it (Chinese remainder theorem), so the other classes
 * need neither be evaluated nor be resident in the proving key.  d_class_remainders: n_classes x n elements, class-major in the
 * order of `classes` (strictly increasing, each < 8); per coefficient index an n_classes x n_classes inverse Vandermonde system in
 * h_k^n is applied (for all 8 classes it is the 8-point inverse DFT above).  d_out: 8n coefficients, the slabs above n_classes
 * zero: the polynomial `coset.ifft` returns at prover.rs:672, provided its degree is below n_classes * n. */
MZK_API int32_t mzk_plonk_quotient_combine_classes_dev(int32_t curve_id, uint32_t log_n, const uint32_t* classes, uint32_t n_classes,
                                                       const void* d_class_remainders, void* d_out, void* stream);
/* ONE class fewer: W classes (5 of the 8 for TurboPlonk, 6 for UltraPlonk).  The W + 3 coefficients of the quotient t from X^(Wn) on
 * are the top coefficients of its numerator (t (X^n - 1) = numerator and deg t = W (n + 1) + 2, so numerator[i] = t[i - n] above
 * that degree; needs n > W + 2), and those are products of the TOP coefficients of the numerator's factors: the two permutation
 * products of prover.rs:741-752 and, for TurboPlonk, the q_ecc / q_hash terms of :696-708 -- everything else lies lower.
 * mzk_plonk_quotient_top_dev computes them on the device (one small kernel; d_polys as for mzk_plonk_quotient_chunked_dev: rows of
 * in_stride elements, the W wire polynomials, then the permutation product, in_len >= n + 3 coefficient slots; key registered by
 * mzk_plonk_pk_register_chunked) into d_top[0 .. W + 3), *out_n_top = W + 3 (nullable).  mzk_plonk_quotient_combine_top_dev subtracts
 * their share h_k^(n n_classes) d_top[j] from the class remainders, solves the n_classes x n_classes system and places d_top in slab
 * n_classes of d_out.  NOTE: the polynomial so recovered has degree W (n + 1) + 2 whatever the witness -- the reference's guard
 * (`WrongQuotientPolyDegree`, prover.rs:915-918) can no longer fire; a host using this path must check the quotient identity itself
 * (both hosts here do, at the evaluation challenge: r(zeta) against the verifier's linearisation constant).  Asynchronous. */
MZK_API int32_t mzk_plonk_quotient_top_dev(uint64_t pk_handle, const void* d_polys, uint64_t in_stride, uint64_t in_len, const uint64_t* alpha_mont,
                                           const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_top, uint32_t* out_n_top, void* stream);
MZK_API int32_t mzk_plonk_quotient_combine_top_dev(int32_t curve_id, uint32_t log_n, const uint32_t* classes, uint32_t n_classes,
                                                   const void* d_class_remainders, const void* d_top, uint32_t n_top, void* d_out, void* stream);

/* ---- preprocess from circuit structure: the permutation half of PlonkKzgSnark::preprocess (plonk/src/proof_system/snark.rs:529-617) ----
 * mzk_plonk_wire_permutation_dev replaces compute_wire_permutation (relation/src/constraint_system.rs:743-778).  d_wire_variables: `cells`
 * u32 variable indices; in a circuit cell c = wire * n + row (cells = W n), but any count below 2^32 is taken (MZK_ERR_UNSUPPORTED at or
 * above).  A variable on the cells c_0 < c_1 < .. < c_(m-1) yields d_out_next_u32[c_i] = c_((i+1) mod m): a variable with one cell maps to
 * itself, variables without a cell are legal (1 <= n_vars).  Field-independent.  The result is a function of the table alone, identical
 * from run to run (a stable radix sort on the variable index: csrc/perm.cuh; no order is left to atomics).  Every index is checked: one
 * >= n_vars makes the call fail with MZK_ERR_INVALID_ARG and mzk_last_error() names the lowest such cell and its value (the reference
 * panics on such an index).  Scratch (16 B per cell) is the context's shared scratch.  Synchronises (it returns the validation result). */
MZK_API int32_t mzk_plonk_wire_permutation_dev(const void* d_wire_variables, uint64_t cells, uint64_t n_vars, void* d_out_next_u32, void* stream);
/* Replaces compute_extended_id_permutation / compute_extended_permutation (relation/src/constraint_system.rs:913-960):
 * d_out[c] = k[next[c] / n] * w^(next[c] mod n) for c < num_wire_types * n, n = 2^log_n, Montgomery, w the primitive n-th root of unity
 * the NTT uses, k_mont the num_wire_types (5 or 6) coset representatives (host): the values of the sigma polynomials on the gate
 * domain, wire-major -- what the inverse NTTs of constraint_system.rs:1162-1195 turn into `ProvingKey::sigmas`.  d_next_u32 from
 * mzk_plonk_wire_permutation_dev over num_wire_types * n cells (< 2^32).  Asynchronous. */
MZK_API int32_t mzk_plonk_sigma_values_dev(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const void* d_next_u32, const uint64_t* k_mont, void* d_out,
                                           void* stream);
/* The way back, for a holder of a `ProvingKey` alone (which carries sigma but not `wire_variables`): the inverses of the two above.
 * mzk_plonk_sigma_decode_dev: d_sigma_values = num_wire_types x n Montgomery elements, wire-major (what mzk_plonk_sigma_values_dev writes,
 * or the forward NTTs of `ProvingKey::sigmas`); for every cell c = wire * n + row the cell (a, b) with sigma[c] = k_a w^b is found and
 * d_out_next_u32[c] = a * n + b.  A hash join against the W n identity values (csrc/unperm.cuh: open addressing, full 32-byte key
 * comparison; scratch: 4 B x the power of two >= 2 W n, the context's shared scratch).  Synchronises.  MZK_ERR_INVALID_ARG, with
 * mzk_last_error() naming the lowest offending cell: a sigma value that is no identity value ("cell <c>: not k_a w^b"), or identity values
 * that collide because the cosets k_a H are not disjoint (named as such).  MZK_ERR_UNSUPPORTED: num_wire_types * n >= 2^32. */
MZK_API int32_t mzk_plonk_sigma_decode_dev(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const void* d_sigma_values, const uint64_t* k_mont,
                                           void* d_out_next_u32, void* stream);
/* A wire-variable table from a permutation of `cells` cells (< 2^32: MZK_ERR_UNSUPPORTED at or above): cells in one cycle share a
 * variable, in CANONICAL numbering -- the variable of a cell is the number of cycle minima below the minimum cell of its cycle, i.e.
 * scanning the cells in order, the first unseen cell gets the next number; *out_n_vars = the number of cycles.  The compute_wire_permutation
 * of that table is d_next_u32 again up to the order inside a cycle, and its copy constraints are the same.  Field-independent.
 * d_next_u32 is validated: MZK_ERR_INVALID_ARG names the lowest cell holding an entry >= cells, else the lowest cell that is the
 * successor of no cell (not a permutation).  Cycle minima by pointer doubling (csrc/unperm.cuh): ceil(log2(longest cycle)) + 1 passes
 * over 16 B per cell of the context's shared scratch, the same work per pass whatever the cycle lengths; no order is left to atomics,
 * the table is a function of d_next_u32 alone.  Synchronises. */
MZK_API int32_t mzk_plonk_variables_from_permutation_dev(const void* d_next_u32, uint64_t cells, void* d_out_variables_u32, uint64_t* out_n_vars, void* stream);

/* Round 2: replaces Arithmetization::compute_prod_permutation_polynomial
 * (relation/src/constraint_system.rs:1197-1223), whose loop performs one field division per gate.
 * wire_values: 5 x n (UltraPlonk key: 6 x n) wire evaluations witness[wire_variable(i, j)]; the sigma evaluations
 * come from the registered proving key.  out: the n coefficients of the permutation product polynomial (unmasked). */
MZK_API int32_t mzk_plonk_perm_product_dev(uint64_t pk_handle, const void* d_wire_values, const uint64_t* beta_mont,
                                           const uint64_t* gamma_mont, void* d_out, void* stream);
MZK_API int32_t mzk_plonk_perm_product(uint64_t pk_handle, const uint64_t* wire_values, const uint64_t* beta_mont,
                                       const uint64_t* gamma_mont, uint64_t* out);

/* The gather of `Arithmetization::compute_wire_polynomials` (relation/src/constraint_system.rs:1225-1247: `self.witness[var]` for
 * every cell of `self.wire_variables[i]`) on the device: d_out[t] = d_witness[d_wire_variables[t]], t < count = W x n, 32-byte field
 * elements of either curve, d_wire_variables = u32 variable indices (wire-major).  The index table is circuit structure -- resident
 * once per circuit -- so a host-resident witness crosses PCIe as n_vars x 32 B instead of W x n x 32 B (the bench circuit: 1 / 5).
 * An index >= n_vars yields zero and is NOT reported here (the call is asynchronous): the reference panics on such an index, so validate
 * the table once where it is registered -- mzk_prover_set_wire_variables does (MZK_ERR_INVALID_ARG).  Asynchronous; the wire iNTTs (mzk_ntt_dev) follow on the same stream. */
MZK_API int32_t mzk_plonk_gather_witness_dev(const void* d_witness, uint64_t n_vars, const void* d_wire_variables, uint64_t count, void* d_out,
                                             void* stream);

/* ---- dense-polynomial primitives of prover rounds 4 and 5 on device-resident coefficient vectors ----
 * evaluate: `DensePolynomial::evaluate` (plonk/src/proof_system/prover.rs:216-235): `batch` polynomials of
 * `len` coefficients, `batch_stride` elements apart, all at the point x; out_mont: batch x 4 limbs on the
 * HOST (the call synchronises). */
MZK_API int32_t mzk_poly_eval_dev(int32_t curve_id, const void* d_coeffs, uint64_t len, uint32_t batch, uint64_t batch_stride,
                                  const uint64_t* x_mont, uint64_t* out_mont, void* stream);
/* Evaluations of several (batches of) polynomials at up to two points in ONE call and one synchronisation: job j evaluates batches[j]
 * polynomials of lens[j] coefficients, strides[j] elements apart from d_coeffs[j], at x_mont[which_x[j]] (which_x[j] is 0 or 1; x_mont
 * holds two elements, the second may repeat the first); out_mont receives the values job after job (sum of batches[] elements).  What
 * round 4 of the prover needs (prover.rs:216-299: everything at zeta and at zeta * omega).  At most 64 jobs. */
MZK_API int32_t mzk_poly_eval_many_dev(int32_t curve_id, uint32_t n_jobs, const void* const* d_coeffs, const uint64_t* lens, const uint32_t* batches,
                                       const uint64_t* strides, const uint32_t* which_x, const uint64_t* x_mont, uint64_t* out_mont, void* stream);
/* out[j] = sum_k scalars[k] * polys[k][j], j < out_len (a polynomial shorter than out_len counts as zero beyond its
 * length): `mul_poly` and the polynomial additions of prover.rs:302-358, 497-501, 1115-1122.  At most 32 terms;
 * d_out may be one of the inputs.  scalars_mont: n_terms x 4 limbs, host.  Asynchronous. */
MZK_API int32_t mzk_poly_lincomb_dev(int32_t curve_id, uint32_t n_terms, const void* const* d_polys, const uint64_t* lens,
                                     const uint64_t* scalars_mont, void* d_out, uint64_t out_len, void* stream);
/* `Prover::mask_polynomial` (prover.rs:463-486) for up to 8 polynomials in one launch: d_polys[i] holds n coefficients in a row
 * of at least n + n_blinders slots; p += (b_0 + b_1 X + ..)(X^n - 1), i.e. p[j] -= b_j and p[n + j] = b_j.  blinders_mont:
 * n_polys x n_blinders x 4 limbs, host (the `DensePolynomial::rand` draws, 1 <= n_blinders <= 4).  Asynchronous. */
MZK_API int32_t mzk_poly_mask_dev(int32_t curve_id, uint32_t n_polys, void* const* d_polys, uint64_t n, uint32_t n_blinders,
                                  const uint64_t* blinders_mont, void* stream);
/* `split_quotient_polynomial` (prover.rs:902-960) in one launch: the W (n + 1) + 3 coefficients at d_quot (the quotient's expected degree is
 * W (n + 1) + 2, W = n_parts, 2..8) into n_parts rows of out_stride (>= n + 3) slots at d_out: row i holds the coefficients
 * [i (n + 2), (i + 1)(n + 2)) -- the last row what is left -- plus the blinder b_i as coefficient n + 2 (rows before the last) minus
 * b_{i-1} in the constant term (rows after the first); every other slot of a row is zeroed.  blinders_mont: (n_parts - 1) x 4 limbs, host.
 * d_out must not overlap d_quot.  Asynchronous. */
MZK_API int32_t mzk_poly_split_quotient_dev(int32_t curve_id, const void* d_quot, uint64_t n, uint32_t n_parts, const uint64_t* blinders_mont,
                                            void* d_out, uint64_t out_stride, void* stream);
/* quotient of p(X) / (X - z), len - 1 coefficients into d_out (remainder dropped, as ark-poly's `/` does at
 * prover.rs:504-506).  d_out must not alias d_poly.  Asynchronous. */
MZK_API int32_t mzk_poly_div_linear_dev(int32_t curve_id, const void* d_poly, uint64_t len, const uint64_t* z_mont, void* d_out, void* stream);
/* The same division, and the remainder p(z) -- which its suffix sums hold anyway -- into *d_rem (one element, device).  The opening
 * proof's batch polynomial divided at zeta leaves (linearisation polynomial)(zeta) + sum_i v^i eval_i there: what a prover needs to
 * check the quotient identity at zeta itself (mzk_plonk_quotient_top_dev). */
MZK_API int32_t mzk_poly_div_linear_rem_dev(int32_t curve_id, const void* d_poly, uint64_t len, const uint64_t* z_mont, void* d_out, void* d_rem,
                                            void* stream);
/* *d_out_len (a u64 in DEVICE memory) = number of coefficients up to and including the highest non-zero one, 0 for the zero
 * polynomial: `DensePolynomial::degree` + 1 after `from_coefficients_vec` has stripped the trailing zeros.  The prover's only
 * guard against an unsatisfied witness is `quot_poly.degree() != expected_degree => WrongQuotientPolyDegree`
 * (plonk/src/proof_system/prover.rs:915-918).  Field-independent (an element is zero iff its 32 bytes are).  Asynchronous:
 * read the word back (mzk_dev_download) once the stream has been synchronised anyway. */
MZK_API int32_t mzk_poly_degree_dev(const void* d_poly, uint64_t len, uint64_t* d_out_len, void* stream);
/* floor quotient of p(X) by the vanishing polynomial of a proof-linking domain, Z_D(X) = prod_{i < count} (X - w^(first + i))
 * with w the primitive 2^log_order-th root of unity (GroupLayout{alignment = log_order, offset = first, size = count},
 * relation/src/proof_linking/mod.rs:16-54): len - count coefficients into d_out, remainder dropped.  Replaces
 * compute_vanishing_polynomial + `&diff / &vanishing_poly` of compute_linking_quotient
 * (plonk/src/proof_system/proof_linking.rs:119-158).  When p vanishes on the whole domain (a valid link) the quotient comes
 * from two coset NTTs and a pointwise 1 / Z_D(x); otherwise the linear factors are divided out one by one -- same
 * coefficients either way.  d_out must not alias d_poly.  The call synchronises the stream (it reads p at the roots). */
MZK_API int32_t mzk_poly_div_roots_dev(int32_t curve_id, const void* d_poly, uint64_t len, uint32_t log_order, uint64_t first, uint64_t count,
                                       void* d_out, void* stream);
/* UnivariateKzgPCS::batch_open (univariate_kzg/mod.rs:163-190, "a naive approach" there) in one pass: K polynomials resident on the device
 * (d_polys[i]: lens[i] Montgomery Fr coefficients, low order first; ragged) opened at points_mont[i] (host, K x 4 limbs) ->
 * out_proofs_xy_mont (host, K affine points x || y, Montgomery, (0, 0) = infinity) and out_evals_mont (host, K x 4 limbs, p_i(z_i)).
 * For all K at once one kernel family (grid.y = polynomial) computes the witness coefficients q_k = c_{k+1} + z q_{k+1} and
 * p(z) = c_0 + z q_0 as a scan of affine maps that share the multiplier z -- no inverse of z and no power tables, so z = 0 is no special
 * case -- and the K witnesses go through ONE batch MSM (as mzk_msm_batch_dev: len - 1 points from base offset 0 each; zero
 * coefficients, leading ones included, contribute nothing), the only place where the call waits: once per fused group of that MSM -- up to
 * six polynomials of one window size -- and not once per polynomial.  The witness scratch comes from the shared
 * workspace; past the budget (1 GiB, or MZK_OPEN_BATCH_BUDGET bytes, read at every call) the polynomials are processed in chunks, each
 * with its own MSM and wait.  lens[i] = 0: proof O, evaluation 0; lens[i] = 1: proof O, evaluation c_0.
 * lens[i] - 1 above the SRS: MZK_ERR_INVALID_ARG, the degree guard of mzk_msm.  Synchronises the stream. */
MZK_API int32_t mzk_kzg_open_batch_dev(uint64_t srs_handle, uint32_t K, const void* const* d_polys, const uint64_t* lens, const uint64_t* points_mont,
                                       uint64_t* out_proofs_xy_mont, uint64_t* out_evals_mont, void* stream);
/* UnivariatePCS::multi_open_rou / _proofs / _evals (univariate_kzg/mod.rs:298-377, pcs/mod.rs:281-306): ONE polynomial resident on the device
 * (d_poly: len Montgomery Fr coefficients, low order first) opened at the first num_points points w^0, w^1, .. of the radix-2 domain of
 * N = 2^log_domain points -> out_proofs_xy_mont (host, affine points x || y, Montgomery, (0, 0) = infinity) and out_evals_mont (host, 4 limbs
 * each, p(w^i)).  num_points above N is clamped to N (the reference's `take`).  Either output may be NULL: without proofs the call is one
 * scalar NTT and touches no SRS point; without evaluations it is the proofs alone.
 * The proofs come from FK23 as the reference's compute_h_poly_in_fk23 and ToeplitzMatrix::fast_vec_mul have it, in O(d log d) group
 * operations: d = next_power_of_two(max(len, 1) - 1) with next_power_of_two(0) = 1, the coefficients padded to d + 1;
 * the points S_k = point srs_offset + k of the SRS, k < d, as the vector [S_(d-1), .., S_0, O^d], whose group NTT of size 2d is kept on the SRS
 * handle for the last (srs_offset, d) asked for -- built on the first call, counted as table bytes by mzk_srs_hbm_bytes, freed by
 * mzk_srs_release --; then a scalar NTT of the circulant column [f_d, 0^(d-1), f_d, f_1, .., f_(d-1)], 2d scalar multiplications, the inverse
 * group NTT, whose first d outputs are the coefficients h of the proof polynomial, and the group NTT of h over the N points.  Nothing is affine
 * between the steps.  d follows len AS GIVEN: trailing zero coefficients are not trimmed -- the proofs are the same points either way, only
 * the number of SRS points the call asks for differs.  len = 0 and len = 1: every proof O; evaluations 0 and c_0.
 * Refused before any launch -- MZK_ERR_INVALID_ARG: fewer than d points from srs_offset on; d > N when proofs are asked for; len > N when
 * evaluations are asked for (the reference: "can't be evaluated on a smaller domain").  MZK_ERR_UNSUPPORTED: log2(2d) (proofs) or log_domain
 * above the two-adicity of Fr, or above 21.  The cap follows the scratch, which comes from the shared workspace and is handed back when
 * the call had to grow it: 2d + N + 8 max(2d, N / 2) XYZZ points (224 B on BLS12-381, 144 B on BN254) for the two arrays and the window tables of
 * the scalar multiplications -- 4.7 GB at 2d = N = 2^21 on BLS12-381, beside the 0.47 GB the handle keeps.  Synchronises the stream. */
MZK_API int32_t mzk_kzg_multi_open_rou_dev(uint64_t srs_handle, uint64_t srs_offset, const void* d_poly, uint64_t len, uint32_t log_domain,
                                           uint64_t num_points, uint64_t* out_proofs_xy_mont, uint64_t* out_evals_mont, void* stream);

/* ---- ADVZ verifiable information dispersal: VidScheme for Advz<E, Sha256> (primitives/src/vid/advz.rs; csrc/vid.hip, vid.cuh, sha256.cuh;
 *      DESIGN.md section 4.17).  A payload becomes K = ceil(elements / payload_chunk_size) polynomials of payload_chunk_size (k) coefficients;
 *      each of the num_storage_nodes (n >= k) nodes receives the K evaluations at its point w^i of the domain of 2^log_domain points
 *      (UnivariatePCS::multi_open_rou_eval_domain(k, n): the chunk size passed where a degree is expected), a path in a ternary SHA-256
 *      tree over the n evaluation vectors, and ONE opening proof of the aggregate polynomial s * sum_j poly_j.  What is restated as the
 *      reference has it, quirks included, and what is unpinned: DESIGN.md section 4.17. ---- */
/* SHA-256 (FIPS 180-4) of len bytes -> out32.  Host only: no GPU, no mzk_init. */
MZK_API int32_t mzk_sha256(const uint8_t* msg, uint64_t len, uint8_t* out32);
/* expand_message_xmd of RFC 9380 section 5.3.1 over SHA-256: out_len <= 8160 bytes from (msg, dst), dst_len <= 255, with Z_pad of z_pad_len
 * zero bytes (<= 4096) in front of msg: 64 is the RFC's (SHA-256's block); ark-ff 0.4's DefaultFieldHasher uses the bytes per field element,
 * 48 for both scalar fields -- the value mzk_hash_to_field_sha256 and the VID scheme use (csrc/sha256.cuh XMD_Z_PAD_ARK).  Host only. */
MZK_API int32_t mzk_expand_message_xmd_sha256(const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint32_t z_pad_len, uint8_t* out,
                                              uint64_t out_len);
/* <DefaultFieldHasher<Sha256, 128> as HashToField<Fr>>::new(dst).hash_to_field(msg, 1)[0]: 48 expanded bytes, big-endian, mod r -> out_mont (4
 * limbs, Montgomery).  Host only. */
MZK_API int32_t mzk_hash_to_field_sha256(int32_t curve_id, const uint8_t* msg, uint64_t len, const uint8_t* dst, uint64_t dst_len, uint64_t* out_mont);
/* bytes_to_field (utilities/src/conversion.rs:379-408) on the device: len bytes at d_bytes (any alignment) -> len / 31 elements of 31 little-endian
 * bytes each and, when 31 does not divide len, the zero-extended last group followed by one element holding its byte count -- len / 31 +
 * (len % 31 ? 2 : 0) Montgomery elements at d_out_mont (16-byte aligned).  A multiple of 31 gets NO length element, as in the reference.  One
 * thread per element; asynchronous on the stream; no scratch.  len >= 2^40: MZK_ERR_INVALID_ARG. */
MZK_API int32_t mzk_bytes_to_field_dev(int32_t curve_id, const void* d_bytes, uint64_t len, void* d_out_mont, void* stream);
/* field_to_bytes (conversion.rs:443-523) as written: count = 1 -> the element's low 31 bytes; otherwise 31 bytes of each of the first count - 2
 * elements, then min(low 64 bits of the LAST element, 32) bytes of the one before it.  It inverts mzk_bytes_to_field_dev for len % 31 != 0 and
 * for len = 0 and 31; for other multiples of 31 it reads the last data element as a length, as the reference does.  d_out_bytes holds at least
 * 31 * max(count - 2, 0) + 32 bytes; *out_len (host) = the bytes written.  8 bytes of the shared workspace.  Synchronises the stream. */
MZK_API int32_t mzk_field_to_bytes_dev(int32_t curve_id, const void* d_elems_mont, uint64_t count, void* d_out_bytes, uint64_t* out_len, void* stream);
/* VidScheme::commit_only: SHA256(C_0 || C_1 || ..) over the ark uncompressed G1 records (as mzk_srs_serialize writes them, infinity included) of
 * the K commitments of the payload's polynomials -- polynomial j = elements j k .. of d_elems_mont (n_elems Montgomery elements on the device, 16-byte
 * aligned), the last one over its own, fewer, coefficients -- by one mzk_msm_batch_dev over the SRS view (srs_offset, srs_len).  n_elems = 0:
 * SHA256 of nothing.  Refused before any launch -- MZK_ERR_INVALID_ARG: k = 0, n < k, the view outside the SRS or shorter than k points, 2^log_domain < n;
 * MZK_ERR_UNSUPPORTED: log_domain above the caps of mzk_kzg_multi_open_rou_dev, 2^24 polynomials.  Scratch: K (point + record) bytes of the shared workspace.
 * Synchronises the stream. */
MZK_API int32_t mzk_vid_advz_commit_only_dev(uint64_t srs_handle, uint64_t srs_offset, uint64_t srs_len, const void* d_elems_mont, uint64_t n_elems,
                                             uint32_t payload_chunk_size, uint32_t num_storage_nodes, uint32_t log_domain, uint8_t* out_commit32, void* stream);
/* Advz::disperse_from_elems (advz.rs:279-391).  In: the payload's elements on the device.  Out, all to the host:
 *   out_commits_xy_mont  K affine points x || y (Montgomery, (0, 0) = infinity): Common::poly_commits
 *   out_evals            n x K x 32 bytes: evals[i][j] = poly_j(w^i) as its canonical little-endian bytes, Share i's `evals`
 *   out_proofs_xy_mont   n affine points: Share i's aggregate_proof, the opening of s * sum_j poly_j at w^i (FK23, mzk_kzg_multi_open_rou_dev)
 *   out_nodes            every digest of the tree, 32 bytes each, level by level: the n leaves SHA256(u64_le(i) || u64_le(K) || evals[i]), then
 *                        ceil(n / 3) branches SHA256(c0 || c1 || c2) (32 zero bytes for a missing child), .. -- height = ilog3(n) + 1 branch
 *                        levels, the root last: sum over the levels of their sizes n, ceil(n / 3), .., 1 (a caller cuts the n paths out of it)
 *   out_commit32         SHA256 of the commitments' uncompressed records (the VID commitment); out_root32: Common::all_evals_digest
 *   out_scalar_mont      s = hash_to_field(SHA256(records || root), DST "rick"), 4 limbs
 * Two phases on the stream around the one forced wait (the host hashes the commitments between them): [zero-padded copy -> batched forward NTT ->
 * leaf kernel (one read of the NTT output writes evals[i][j] and hashes it) -> one launch per tree level -> batch MSM], then [aggregate -> FK23].
 * n_elems = 0 is a valid dispersal: K = 0, leaves of 16 bytes, every proof O.  Refusals: those of mzk_vid_advz_commit_only_dev, before any
 * launch.  Scratch from the shared workspace, in bytes: 32 (K 2^log_domain + n K + nodes + k) + K (point + record) -- beside what the batch MSM and
 * mzk_kzg_multi_open_rou_dev take.  Synchronises the stream. */
MZK_API int32_t mzk_vid_advz_disperse_dev(uint64_t srs_handle, uint64_t srs_offset, uint64_t srs_len, const void* d_elems_mont, uint64_t n_elems,
                                          uint32_t payload_chunk_size, uint32_t num_storage_nodes, uint32_t log_domain, uint64_t* out_commits_xy_mont,
                                          uint8_t* out_evals, uint64_t* out_proofs_xy_mont, uint8_t* out_nodes, uint8_t* out_commit32, uint8_t* out_root32,
                                          uint64_t* out_scalar_mont, void* stream);
/* The Merkle half of Advz::verify_share for n_shares shares in ONE launch, one thread per share (all arguments on the host): share t has
 * indices[t], evals[t] (evals_per_share x 32 canonical little-endian bytes) and paths[t] (height levels from the leaf up, the 2 sibling digests of
 * each level in child order, zeros for an empty one; height = ilog3(num_storage_nodes) + 1).  out_ok[t] = 1 when indices[t] < num_storage_nodes
 * and the leaf hashed from evals[t] climbs to root32 with the index's base-3 digits, least significant first, as the traversal key;
 * out_agg_evals_mont[t] = s * sum_j evals[t][j] (4 limbs, Montgomery): the value the share's KZG opening is checked against
 * (UnivariateKzgPCS::verify at w^index).  n_shares = 0: nothing.  Scratch: the arguments' bytes + 36 n_shares.  Synchronises the stream. */
MZK_API int32_t mzk_vid_advz_verify_shares_dev(int32_t curve_id, uint64_t n_shares, uint64_t evals_per_share, uint32_t num_storage_nodes, const uint64_t* indices,
                                               const uint8_t* evals, const uint8_t* paths, const uint8_t* root32, const uint64_t* scalar_mont, int32_t* out_ok,
                                               uint64_t* out_agg_evals_mont, void* stream);
/* Advz::recover_elems' interpolation (reed_solomon_erasure_decode_rou, reed_solomon_code/mod.rs:68-187): k = payload_chunk_size shares with
 * indices[i] (host) and evals_mont[p][i] (host, n_polys x k Montgomery elements: polynomial p at w^indices[i]) -> d_out_mont (device, 16-byte
 * aligned): n_polys x k coefficients, polynomial after polynomial.  The interpolant is unique, so the field elements are the reference's: the k x k
 * matrix of the Lagrange basis is built once (master polynomial in one workgroup, l'(x_i), one inversion and a synthetic division per row),
 * then out[p][c] = sum_i y[p][i] M[i][c] with n_polys k threads.  Refused before any launch -- MZK_ERR_INVALID_ARG: k = 0, an index >= 2^log_domain,
 * a duplicate index; MZK_ERR_UNSUPPORTED: k > 1024, the one workgroup (and 32 KiB of LDS) of the master polynomial.  Scratch: 32 (2 k + k^2 + n_polys k)
 * bytes of the shared workspace, 32 MiB for the matrix at the cap.  Synchronises the stream. */
MZK_API int32_t mzk_vid_advz_recover_dev(int32_t curve_id, uint32_t payload_chunk_size, uint64_t n_polys, uint32_t log_domain, const uint64_t* indices,
                                         const uint64_t* evals_mont, void* d_out_mont, void* stream);

/* ---- the prover's rounds on device-resident state: replaces the BODIES of Prover::run_1st_round .. compute_opening_proofs
 *      (plonk/src/proof_system/prover.rs:72-419) as PlonkKzgSnark::batch_prove_internal calls them (snark.rs:263-431).
 * One mzk_prover per (proving key, instance slot): it holds, in HBM, the coefficient forms of the key's fixed polynomials, their
 * evaluations on the residue classes of the quotient domain that the quotient needs (mzk_plonk_pk_register_chunked) -- the key part,
 * which mzk_prover_fork shares among several handles -- and owns the workspace of one proof in flight (`Oracles`, structs.rs:875-887).  The CALLER keeps what the reference's snark.rs keeps: the
 * transcript (challenges in, commitments / evaluations out), the rng (blinders in, in the reference's draw order: SURVEY.md
 * Appendix C) and the `Proof` struct.  Nothing but challenges, blinders, public inputs, commitments (affine x||y, mont; (0,0) =
 * infinity: `Commitment(G1Affine)`) and evaluations crosses the boundary per round; the witness crosses once (or not at all:
 * MZK_WITNESS_DEV_*).  All field elements Montgomery, 4 limbs.
 *
 *   reference                                          here
 *   Prover::new + ProvingKey (structs.rs:575-590)       mzk_prover_create
 *   run_1st_round          prover.rs:72-87             mzk_prover_round1        -> W wire commitments
 *   run_plookup_1st_round  prover.rs:89-118            mzk_prover_round1_5      -> h_1, h_2 commitments          (UltraPlonk)
 *   run_2nd_round          prover.rs:125-141           mzk_prover_round2        -> permutation-product commitment
 *   run_plookup_2nd_round  prover.rs:143-183           mzk_prover_round2_5      -> Plookup-product commitment    (UltraPlonk)
 *   run_3rd_round          prover.rs:192-209           mzk_prover_round3        -> W split-quotient commitments  (all instances)
 *   compute_evaluations (+ plookup)  prover.rs:216-299 mzk_prover_round4        -> ProofEvaluations (+ PlookupEvaluations)
 *   compute_(non_)quotient_component_for_lin_poly + compute_opening_proofs  prover.rs:302-460
 *                                                      mzk_prover_round5        -> opening proof, shifted opening proof (all instances)
 *
 * Rounds must be called in this order (MZK_ERR_STATE otherwise); a new mzk_prover_round1 starts the next proof on the same handle.
 * `batch_prove` over K instances: K handles (one per instance, same domain size and curve), rounds 1 - 2.5 and 4 per handle,
 * rounds 3 and 5 once with all handles (alpha_base_k = alpha^(3k), alpha^(7k) with Plookup: prover.rs:661-669, snark.rs:408-428).
 *
 * Unsatisfied witness: the reference's only guard is `WrongQuotientPolyDegree` (prover.rs:915-918), raised in round 3.  Here the
 * quotient is recovered from W residue classes and the top coefficients of its numerator (mzk_plonk_quotient_top_dev), which has
 * the expected degree whatever the witness; the guard is the quotient identity at zeta, checked at the end of round 5 on a value
 * the opening's division leaves anyway: mzk_prover_round5 returns MZK_ERR_WRONG_QUOTIENT_DEGREE (the proof must be discarded).
 * Tiny domains (n <= W + 2) keep the reference's guard and round 3 returns that code.
 *
 * Streams (round 5).  A handle runs its rounds on a non-blocking stream of its device context (two per context, handed to its handles in
 * turn; MZK_PROVER_NULL_STREAM=1: the null stream, as before).  mzk_prover_round1 makes that stream wait for everything the caller has
 * enqueued on the NULL stream (a device-resident witness written there is complete first; work on other streams of the caller's must be
 * synchronised by the caller); every round returns when its outputs are in host memory; mzk_prover_poly_dev's pointers are valid to read
 * on any stream once round 5 has returned.  Two proofs on one card -- two host threads, each bound (mzk_init) to its own device context
 * (MZK_VIRTUAL_DEVICES maps several contexts onto one GPU), or two handles of one context -- run concurrently where the hardware allows.
 * A prover and its forks (mzk_prover_fork) are such handles of one context, and may run their rounds from different host threads: the
 * key part they share is read-only once a second handle holds it, every handle has its own workspace, state and stream, and enqueueing is
 * under the context's device lock as for any two handles of one context.  One handle still belongs to one thread at a time, and
 * mzk_prover_fork / mzk_prover_set_wire_variables / mzk_prover_derive_wire_variables / mzk_prover_destroy of a handle must not run concurrently with
 * each other on that handle.
 * Domains whose quotient does not fit the 8n-point domain (num_wire_types * (n + 1) + 2 >= 8 n: n = 2; n = 4 with six wire types) are
 * refused by mzk_prover_create with MZK_ERR_UNSUPPORTED. */
#define MZK_ERR_WRONG_QUOTIENT_DEGREE (-9) /* PlonkError::WrongQuotientPolyDegree: the witness does not satisfy the circuit */
#define MZK_ERR_STATE (-10)                /* prover rounds called out of order */
#define MZK_ERR_ENCODING (-11)             /* invalid point encoding: mzk_last_error() = "point <i>: <reason>" (mzk_srs_register_serialized); a serialized key
                                            * that is refused: "<field> ..: <reason>" (mzk_key_layout, mzk_fr_decode_dev, mzk_prover_create_serialized) */

/* Several devices / processes: this prover is rank `rank` of `world` -- it commits over the SRS points
 * [rank (n+3) / world ..) of every polynomial, evaluates ceil(W / world) residue classes of the quotient, runs rounds 4-5 on its
 * coefficient range.  The callbacks move a few hundred bytes through host memory (Jacobian partial sums of 144 / 96 B, field elements
 * of 32 B); every rank ends each round with the SAME commitments and evaluations.  all_gather: every rank's `bytes` bytes,
 * concatenated in rank order, into recv (world x bytes).  exchange_classes (nullable): make the class remainders of all ranks
 * resident in d_rem (n_classes x class_bytes, device; this rank has filled [first_own, first_own + n_own)); NULL = the prover pushes
 * its own classes into the peers' buffers itself (mzk_prover_set_peer_buffers, hipMemcpyPeerAsync over xGMI) and calls barrier.
 * Callbacks return 0 on success.  FAILURE: a rank whose round fails (bad argument, MZK_ERR_WRONG_QUOTIENT_DEGREE, a HIP error) returns
 * without entering the round's remaining collectives, so its peers would wait in all_gather / barrier for ever: the CALLER's
 * collectives must be abortable or time out (the in-tree LocalComm has an abort flag every waiter polls; torch.distributed callers set
 * a process-group timeout), and a non-zero return of a callback ends the round on that rank with MZK_ERR_INVALID_ARG. */
typedef struct mzk_comm {
    void* ctx;
    int32_t rank, world;
    int32_t (*all_gather)(void* ctx, const void* send, uint64_t bytes, void* recv);
    int32_t (*barrier)(void* ctx);
    int32_t (*exchange_classes)(void* ctx, void* d_rem, uint64_t class_bytes, uint32_t first_own, uint32_t n_own, uint32_t n_classes);
} mzk_comm;

/* selector_coeffs: nsel x poly_len (nsel = 13, or 14 with q_lookup last: num_wire_types 6), sigma_coeffs: W x poly_len, table_coeffs:
 * 4 x poly_len (range, key, table_dom_sep, q_dom_sep; NULL for TurboPlonk): `ProvingKey{selectors, sigmas, plookup_pk}` as
 * DensePolynomial coefficient vectors, low order first, poly_len <= n = 2^log_n (host).  k_mont: the W coset representatives `vk.k`.
 * commit_key: SRS handle with >= n + 3 points (`pk.commit_key`, trim(n + 2): snark.rs:535, 561).  lagrange_key: 0, or a handle from
 * mzk_srs_lagrange_from_srs(commit_key, log_n, 3): round 1 (and 1.5) then commit the wire VALUES over the Lagrange basis -- same
 * group elements, mostly small scalars.  comm: NULL = one device.  The prover lives on the calling thread's device.
 * With a comm, commit_key (and lagrange_key) may instead hold ONLY this rank's point range [rank (n+3) / world ..) -- exactly that many points
 * (mzk_srs_slice): the rank then keeps 1 / world of the SRS and of its fixed-base table. */
MZK_API int32_t mzk_prover_create(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const uint64_t* selector_coeffs,
                                  const uint64_t* sigma_coeffs, const uint64_t* table_coeffs, uint64_t poly_len, const uint64_t* k_mont,
                                  uint64_t commit_key, uint64_t lagrange_key, const mzk_comm* comm, uint64_t* out_prover);
/* The same prover from what a FINALISED CIRCUIT holds -- the whole of PlonkKzgSnark::preprocess (snark.rs:529-617) on the device:
 * compute_wire_permutation, compute_extended_permutation and the 13 + W (+ 4) inverse FFTs of compute_selector_polynomials /
 * compute_extended_permutation_polynomials (relation/src/constraint_system.rs:743-778, 913-960, 1162-1195) and of the Plookup table
 * polynomials.  selector_values: nsel x n VALUES on the gate domain (selector order as above), wire_variables: W x n u32 variable indices
 * (wire-major, every entry < n_vars, 1 <= n_vars < 2^32; checked, MZK_ERR_INVALID_ARG names the lowest offending cell), table_values:
 * 4 x n values (range, key, table_dom_sep, q_dom_sep) or NULL for TurboPlonk.  Wire permutation -> sigma values -> one batched inverse
 * NTT over all nsel + W (+ 4) rows -> everything mzk_prover_create does, from coefficient forms that never leave the device.  The
 * variable table stays resident exactly as after mzk_prover_set_wire_variables: the *_VECTOR witness kinds work at once and
 * mzk_prover_check_witness checks the copy constraints of every witness kind.  comm as for mzk_prover_create: every rank computes the
 * same key, there is no collective call.  Set-up peak: (nsel + W (+ 4)) x n x 32 B besides the prover's own memory, handed back before
 * the call returns.  The _dev form takes device arrays, complete on the null stream (or synchronised).  Both synchronise. */
MZK_API int32_t mzk_prover_create_from_circuit(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const uint64_t* selector_values,
                                               const uint32_t* wire_variables, uint64_t n_vars, const uint64_t* table_values, const uint64_t* k_mont,
                                               uint64_t commit_key, uint64_t lagrange_key, const mzk_comm* comm, uint64_t* out_prover);
MZK_API int32_t mzk_prover_create_from_circuit_dev(int32_t curve_id, uint32_t log_n, uint32_t num_wire_types, const void* d_selector_values,
                                                   const void* d_wire_variables, uint64_t n_vars, const void* d_table_values, const uint64_t* k_mont,
                                                   uint64_t commit_key, uint64_t lagrange_key, const mzk_comm* comm, uint64_t* out_prover);
/* The same prover from what a jf-plonk user holds: the CanonicalSerialize image of a `ProvingKey<E>` (format: mzk_key_layout above).
 * flags: MZK_SER_COMPRESSED states the image's mode; MZK_SER_VALIDATE applies to the G1 records of the commit key, as for
 * mzk_srs_register_serialized; MZK_KEY_CHECK_COMMITMENTS below.  The container is parsed on the host (mzk_key_layout), the image staged
 * on the device in ONE copy, all polynomials and k decoded in ONE launch (mzk_fr_decode_dev: range check, Montgomery form, zero fill)
 * into nsel + W (+ 4) rows of n, and the prover built from those rows: the coefficient forms never exist on the host.
 * commit_key == 0: the embedded commit key is registered from the staged bytes (mzk_srs_register_serialized_dev) and its handle returned in
 * *out_commit_key (required then); the caller releases it after the prover.  commit_key != 0: that handle is used, the embedded points
 * are skipped and not compared -- one SRS and its fixed-base table serve many keys -- and *out_commit_key (nullable) is 0.
 * out_lagrange_key non-NULL: the Lagrange-basis key is derived (mzk_srs_lagrange_from_srs(ck, log_n, 3)), given to the prover and returned;
 * the caller releases it too.  The G2 elements and the commitments inside vk are not decoded: they pass through as bytes.
 * MZK_KEY_CHECK_COMMITMENTS: the prover's own commitments (mzk_prover_vk_commitments), encoded in the image's mode ((0, 0) as ark's
 * infinity: the commitment of a zero selector), must equal the records of vk bytewise, and vk.open_key.g commit-key point 0.
 * MZK_ERR_ENCODING: mzk_last_error() names the field -- "sigmas[2] coefficient 5: not below the modulus", "commit_key point 7: not in the
 * subgroup", "vk.selector_comms[3] does not commit selectors[3]", or mzk_key_layout's text -- and *out_bad (nullable) holds the index
 * within the field (UINT64_MAX for container errors).  On any failure no handle exists and nothing stays allocated.  comm: NULL or world 1;
 * world > 1 is MZK_ERR_UNSUPPORTED (sharded loading).  Domain sizes mzk_prover_create refuses are refused alike.  Synchronises.
 * Set-up peak: the staged image (len bytes) plus the rows ((nsel + W (+ 4) + 1) x n x 32 B) besides the prover's own memory and, when
 * it is registered here, the commit key with its decode; both are handed back before the call returns. */
MZK_API int32_t mzk_prover_create_serialized(int32_t curve_id, const uint8_t* bytes, uint64_t len, uint32_t flags, uint64_t commit_key, const mzk_comm* comm,
                                             uint64_t* out_prover, uint64_t* out_commit_key, uint64_t* out_lagrange_key, uint64_t* out_bad);
/* The `ProvingKey` image of ANY prover handle, however it was created (flags: MZK_SER_COMPRESSED or 0): polynomial lengths from
 * mzk_poly_degree_dev on the resident rows (trailing zeros stripped, as from_coefficients_vec does), records from mzk_fr_encode_dev,
 * commitments from mzk_prover_vk_commitments, k and domain_size from the key, g = commit-key point 0, the commit key its first n + 3 points
 * (trim(n + 2)).  What the library does not hold is the caller's: num_inputs, is_merged and the two G2 elements of the open key as bytes of
 * the same mode (g2 record bytes each; copied, not looked at).  out_bytes == NULL: only *out_len, the size, is written (no commitment is
 * computed); else capacity >= that size (MZK_ERR_INVALID_ARG).  mzk_prover_serialize_vk: the `VerifyingKey` image alone -- the vk slice of
 * the former.  MZK_ERR_UNSUPPORTED: the handle's commit key is a rank's slice.  Both synchronise; staging: one row of n records. */
MZK_API int32_t mzk_prover_serialize_key(uint64_t prover, uint32_t flags, uint64_t num_inputs, const uint8_t* h_bytes, const uint8_t* beta_h_bytes,
                                         int32_t is_merged, uint8_t* out_bytes, uint64_t capacity, uint64_t* out_len);
MZK_API int32_t mzk_prover_serialize_vk(uint64_t prover, uint32_t flags, uint64_t num_inputs, const uint8_t* h_bytes, const uint8_t* beta_h_bytes,
                                        int32_t is_merged, uint8_t* out_bytes, uint64_t capacity, uint64_t* out_len);
MZK_API int32_t mzk_prover_destroy(uint64_t prover);
/* Another slot on the same proving key: a new handle on `prover`'s device context that SHARES its key part -- the coefficient forms, the
 * chunked proving key with its resident class evaluations, the SRS handles and the resident variable table -- and owns a fresh
 * workspace, state (the next call must be round 1) and stream (the next of the context's rotation); profiling is off on it.  The
 * reference's batch_prove takes `&[&ProvingKey]` in which one key may appear K times (snark.rs:263-431): here that is a prover and
 * K - 1 forks as the K instances of rounds 3 and 5 (the SAME handle twice is still refused), and the same family serves K proofs in
 * flight on one key.  The call does no SRS work, no NTT and no upload: it allocates the workspace mzk_prover_create allocates.  A fork
 * of a fork is a peer of all the others; handles are destroyed in any order and the key lives until its last holder is gone.  `prover`
 * may have a proof in flight: its state is not touched.  A fork of a prover that has the variable table (mzk_prover_create_from_circuit,
 * or mzk_prover_set_wire_variables before the fork) has it too.  MZK_ERR_BAD_HANDLE: unknown handle; MZK_ERR_INVALID_ARG: null
 * out_prover; MZK_ERR_UNSUPPORTED: `prover` was created with an mzk_comm of world > 1 (two slots would interleave one communicator's
 * collectives); MZK_ERR_OOM: the workspace did not fit, nothing stays allocated. */
MZK_API int32_t mzk_prover_fork(uint64_t prover, uint64_t* out_prover);
/* `VerifyingKey{selector_comms, sigma_comms}` (preprocess, snark.rs:562-594) from the resident coefficient forms: nsel + W affine points,
 * then -- UltraPlonk, out_plookup_xy non-NULL -- range_table_comm, key_table_comm, table_dom_sep_comm, q_dom_sep_comm (:575-590). */
MZK_API int32_t mzk_prover_vk_commitments(uint64_t prover, uint64_t* out_xy_mont, uint64_t* out_plookup_xy_mont);      /* (with a comm: a collective, every rank calls it) */
/* `wire_variables` of the finalised circuit (relation/src/constraint_system.rs:1225-1247), W x n u32 (host), every entry < n_vars (checked:
 * MZK_ERR_INVALID_ARG -- the reference panics on such an index): resident circuit structure for MZK_WITNESS_*_VECTOR.  On a handle that
 * shares its key (mzk_prover_fork) the table is replaced for THAT handle only (copy-on-write): the other handles keep the shared one. */
MZK_API int32_t mzk_prover_set_wire_variables(uint64_t prover, const uint32_t* wire_variables, uint64_t n_vars);
/* The same table recovered from the key itself, for a prover created from coefficient forms (mzk_prover_create): W forward NTTs of the
 * resident sigma polynomials onto the gate domain, mzk_plonk_sigma_decode_dev, mzk_plonk_variables_from_permutation_dev, all in the
 * context's shared scratch, then installed exactly as mzk_prover_set_wire_variables installs one: copy-on-write on a handle that shares
 * its key, counted in mzk_prover_hbm_bytes' workspace, the same concurrency rule, a proof in flight treated the same.  A table the handle
 * already has is replaced; on any error the handle keeps what it had.  Variables are in canonical numbering (above): the representative
 * of a variable -- its smallest cell -- is the minimum of its sigma-cycle, and a *_VECTOR witness holds, at index v, the value on the
 * minimum cell of cycle v (build it from mzk_prover_get_wire_variables).  *out_n_vars (nullable): the number of variables.  With an
 * mzk_comm: no collective call, any rank may call it alone (every rank holds the full coefficient forms).  Synchronises.
 * MZK_ERR_INVALID_ARG: the sigma polynomials are not those of a permutation of the cells (mzk_last_error() as for the two primitives). */
MZK_API int32_t mzk_prover_derive_wire_variables(uint64_t prover, uint64_t* out_n_vars);
/* The resident table, whatever installed it: W x n u32 into out_wire_variables (host; NULL: only *out_n_vars is written), capacity_cells
 * >= W x n.  MZK_ERR_INVALID_ARG: the handle has no table, or capacity_cells is too small.  Synchronises. */
MZK_API int32_t mzk_prover_get_wire_variables(uint64_t prover, uint32_t* out_wire_variables, uint64_t capacity_cells, uint64_t* out_n_vars);
#define MZK_WITNESS_DEV_WIRES 0   /* device, W x n: witness[wire_variable(i, j)] already gathered.  The prover keeps the POINTER, not a copy:
                                   * the buffer must stay valid and unmodified until round 2 (round 2.5 for UltraPlonk) has returned --
                                   * rounds 1.5 and 2 read the wire values again (sorted vector, permutation product) */
#define MZK_WITNESS_HOST_WIRES 1  /* host, W x n (page-locked memory: column k + 1 crosses PCIe under the iNTT of column k) */
#define MZK_WITNESS_HOST_VECTOR 2 /* host, n_vars witness values; gathered on the device (mzk_prover_set_wire_variables) */
#define MZK_WITNESS_DEV_VECTOR 3  /* device, n_vars witness values */
/* Round 1: compute_wire_polynomials (gather + W iNTTs), compute_pub_input_polynomial, mask_polynomial, batch_commit.
 * witness_len: W x n or n_vars elements.  Public input: n_pub values; pub_input_rows = NULL places them on rows 0 .. n_pub - 1 (where
 * finalize_for_arithmetization puts the IO gates), else row pub_input_rows[i] < n.  blinders_mont: W x 2 (`DensePolynomial::rand(1)` per
 * wire, in wire order).  out_comms_xy: W affine points. */
MZK_API int32_t mzk_prover_round1(uint64_t prover, int32_t witness_kind, const void* witness, uint64_t witness_len, const uint64_t* pub_input_rows,
                                  const uint64_t* pub_input_mont, uint64_t n_pub, const uint64_t* blinders_mont, uint64_t* out_comms_xy);
/* Where a witness is wrong (the other half of what the reference's degree guard was used for; cf. "Unsatisfied witness" above):
 * Circuit::check_circuit_satisfiability (relation/src/constraint_system.rs:389-451) for a caller that holds arrays only, with the
 * witness where mzk_prover_round1 takes it -- all four witness kinds, the public input placed as round 1 places it.  Returns MZK_OK
 * whether or not the witness satisfies the circuit: the report carries the answer.  All values in Fr; W = 5 or 6, w_j[i] the value
 * on wire j of row i, selector order as for mzk_prover_create.
 *   gate    row i < n fails iff  pi[i] + q_c + sum_{j<4} q_lc[j] w_j + q_mul[0] w_0 w_1 + q_mul[1] w_2 w_3 + sum_{j<4} q_hash[j] w_j^5
 *           + q_ecc w_0 w_1 w_2 w_3 w_4 - q_o w_4 != 0  (check_gate, :695-738); pi[i] is zero off the public-input rows, so a wrong or
 *           missing public input is a gate failure on its row.  gate_residual is that left-hand side on gate_row.
 *   lookup  (UltraPlonk) the tau-free form of what the Plookup argument enforces: row i < n - 1 passes iff some row j < n has
 *           (range[j], q tds[j], q key[j], q w_3[j], q w_4[j]) = (w_5[i], q' qds[i], q' w_0[i], q' w_1[i], q' w_2[i]),  q = q_lookup[j],
 *           q' = q_lookup[i], tds / qds the table_dom_sep / q_dom_sep tables -- the coefficients in tau of merged_table_value /
 *           merged_lookup_wire_value (:1441-1480): exactly the rows whose merged value round 1.5 finds in the merged table for every
 *           tau.  Row n - 1 is not looked up (:1390-1398) and never fails.  On circuits built by the reference's gadgets this coincides
 *           with check_range_gate (:602-618) plus the key / value check of :405-449.
 *   copy    *_VECTOR kinds: the copy constraints hold by construction (copy_checked = 1, no failures).  *_WIRES kinds with a table from
 *           mzk_prover_set_wire_variables: the representative of a variable is its cell of smallest index wire * n + row; a cell fails
 *           iff its value differs from its representative's; copy_cell is the failing cell of smallest index.  *_WIRES kinds without a
 *           table: copy_checked = 0 and `kind` is decided by the other two families (nothing decodes sigma unless asked).  A prover from
 *           mzk_prover_create_from_circuit has the table; any other gets it from mzk_prover_set_wire_variables or, from its own sigma
 *           polynomials, mzk_prover_derive_wire_variables -- the counts, copy_cell and copy_rep_cell are then those of the circuit's table.
 * Counts and locations are exact and deterministic.  MZK_ERR_INVALID_ARG: null report, wrong witness_len, a *_VECTOR kind without
 * mzk_prover_set_wire_variables, a public-input row >= n.  MZK_ERR_UNSUPPORTED: copy check with W n >= 2^32.
 * The call synchronises, needs no SRS and makes no collective call (with an mzk_comm any rank may call it alone).  Like a new
 * mzk_prover_round1 it abandons a proof in flight on the handle: the next round call must be round 1 (MZK_ERR_STATE otherwise).  For
 * MZK_WITNESS_DEV_WIRES the pointer is not kept.  Scratch is the context's shared scratch (selector values on H from 13 forward NTTs of
 * the resident coefficient forms, hash slots): mzk_prover_hbm_bytes reports the same figures before and after. */
#define MZK_CHECK_SATISFIED 0
#define MZK_CHECK_GATE 1
#define MZK_CHECK_LOOKUP 2
#define MZK_CHECK_COPY 3
typedef struct mzk_witness_report {
    uint32_t kind;          /* 0, or the first failing family in the order gate, lookup, copy */
    uint32_t copy_checked;  /* 1: copy constraints were checked (or hold by construction); 0: they could not be */
    uint64_t gate_failures, gate_row;                  /* rows failing the gate identity; the lowest one (UINT64_MAX if none) */
    uint64_t lookup_failures, lookup_row;              /* UltraPlonk; 0 / UINT64_MAX on TurboPlonk */
    uint64_t copy_failures, copy_cell, copy_rep_cell;  /* cells as wire * n + row; UINT64_MAX if none */
    uint64_t row_wires[6 * 4];                         /* the W wire values (Montgomery) of the row that `kind` reports; rest zero */
    uint64_t gate_residual[4];                         /* kind == GATE: expected_gate_output - q_o * w_4 on gate_row (Montgomery) */
} mzk_witness_report;
MZK_API int32_t mzk_prover_check_witness(uint64_t prover, int32_t witness_kind, const void* witness, uint64_t witness_len,
                                         const uint64_t* pub_input_rows, const uint64_t* pub_input_mont, uint64_t n_pub,
                                         mzk_witness_report* out_report);
/* UltraPlonk only.  blinders: 2 x 3 (h_1 then h_2); out: 2 points.  MZK_ERR_LOOKUP when a looked-up value is not in the table. */
MZK_API int32_t mzk_prover_round1_5(uint64_t prover, const uint64_t* tau_mont, const uint64_t* blinders_mont, uint64_t* out_comms_xy);
/* blinders: 3; out: 1 point. */
MZK_API int32_t mzk_prover_round2(uint64_t prover, const uint64_t* beta_mont, const uint64_t* gamma_mont, const uint64_t* blinders_mont,
                                  uint64_t* out_comm_xy);
/* UltraPlonk only.  blinders: 3; out: 1 point. */
MZK_API int32_t mzk_prover_round2_5(uint64_t prover, const uint64_t* blinders_mont, uint64_t* out_comm_xy);
/* provers: the n_instances handles in instance order (all past round 2 / 2.5).  blinders: W - 1 (split_quotient_polynomial's draws,
 * prover.rs:947-955).  out: W points. */
MZK_API int32_t mzk_prover_round3(const uint64_t* provers, uint32_t n_instances, const uint64_t* alpha_mont, const uint64_t* blinders_mont,
                                  uint64_t* out_comms_xy);
/* out_evals_mont: wires_evals (W), wire_sigma_evals (W - 1), perm_next_eval (1), then for UltraPlonk the 15 PlookupEvaluations in
 * their declaration order (structs.rs:496-541): range_table, key_table, table_dom_sep, q_dom_sep, h_1, q_lookup, prod_next,
 * range_table_next, key_table_next, table_dom_sep_next, h_1_next, h_2_next, q_lookup_next, w_3_next, w_4_next. */
MZK_API int32_t mzk_prover_round4(uint64_t prover, const uint64_t* zeta_mont, uint64_t* out_evals_mont);
/* out: opening_proof, shifted_opening_proof (2 points).  MZK_ERR_WRONG_QUOTIENT_DEGREE: see above. */
MZK_API int32_t mzk_prover_round5(const uint64_t* provers, uint32_t n_instances, const uint64_t* v_mont, uint64_t* out_comms_xy);
/* Multi-device hosts in one process: this rank's class-remainder buffer (device pointer, bytes), and the same buffers of all `world`
 * ranks with their logical devices, for the one device-to-device exchange of round 3 (mzk_comm.exchange_classes == NULL). */
MZK_API int32_t mzk_prover_exchange_buffer(uint64_t prover, void** out_dptr, uint64_t* out_bytes);
MZK_API int32_t mzk_prover_set_peer_buffers(uint64_t prover, void* const* peer_dptrs, const int32_t* peer_devices);
/* A device-resident polynomial of the proof in flight (valid until the next mzk_prover_round1 on this handle): which = 0 .. W - 1 the
 * masked wire polynomials (n + 2 coefficients; wire 0 is the `linking_wire_poly` of prove_with_link_hint, snark.rs:81-119), W the
 * permutation product (n + 3). */
MZK_API int32_t mzk_prover_poly_dev(uint64_t prover, uint32_t which, const void** out_dptr, uint64_t* out_len);
/* on != 0: every round synchronises the device at its internal stage boundaries and records wall milliseconds; mzk_prover_timings writes
 * them as one JSON object ("r1_ntt_mask", "r1_commit", .. "r5_commit") into buf (NUL-terminated, truncated to cap). */
MZK_API int32_t mzk_prover_profile(uint64_t prover, int32_t on);
MZK_API int32_t mzk_prover_timings(uint64_t prover, char* buf, uint64_t cap);
/* Bytes of HBM this prover holds: coefficient forms, resident class evaluations (proving key), per-proof workspace. */
MZK_API int32_t mzk_prover_hbm_bytes(uint64_t prover, uint64_t* out_fixed, uint64_t* out_proving_key, uint64_t* out_workspace);
/* Of the bytes mzk_prover_hbm_bytes reports for this handle -- it reports what the handle REACHES, shared parts included, forked or not --
 * those held in common with other living handles (mzk_prover_fork), and the number of handles on that key, this one included.  One
 * sharer: 0 bytes.  Otherwise out_fixed + out_proving_key + the shared variable table; that table is counted in out_workspace (as it
 * always was) and here, unless this handle has replaced it by one of its own (mzk_prover_set_wire_variables, counted in out_workspace
 * only).  HBM of a family of handles on one key: sum over the handles of (fixed + proving_key + workspace) - (sharers - 1) x shared. */
MZK_API int32_t mzk_prover_shared_hbm_bytes(uint64_t prover, uint64_t* out_shared_bytes, uint32_t* out_sharers);

/* ---- page-locked host memory for the host-pointer entry points (mzk_ntt, mzk_ntt_batch, mzk_msm, mzk_msm_batch) ----
 * A shim that swaps only the two third-party call sites moves every operand over PCIe.  From memory
 * obtained here (hipHostMalloc), or registered in place (hipHostRegister: worth it for long-lived buffers only), the transfers
 * are DMA at link rate and asynchronous, so that inside a batch call -- and between concurrent callers, the reference's Rayon
 * `par_iter`s (plonk/src/proof_system/prover.rs:552-562, primitives/src/pcs/univariate_kzg/mod.rs:125-127) -- the upload of
 * polynomial k+1 and the download of k-1 overlap the transform of k.  Pageable memory works too, staged by the runtime. */
MZK_API int32_t mzk_host_alloc(uint64_t bytes, void** out_ptr);
MZK_API int32_t mzk_host_free(void* ptr);
MZK_API int32_t mzk_host_register(void* ptr, uint64_t bytes);
MZK_API int32_t mzk_host_unregister(void* ptr);

/* ---- device memory helpers for bindings without HIP of their own ---- */
MZK_API int32_t mzk_dev_alloc(uint64_t bytes, void** out_dptr);
MZK_API int32_t mzk_dev_free(void* dptr);
MZK_API int32_t mzk_dev_upload(void* dptr, const void* host, uint64_t bytes);
MZK_API int32_t mzk_dev_download(void* host, const void* dptr, uint64_t bytes);
MZK_API int32_t mzk_dev_sync(void);
/* Non-blocking streams of the calling thread's device and asynchronous transfers on them (page-locked host memory: mzk_host_alloc),
 * for a host that overlaps the upload of witness column k + 1 with the iNTT of column k (the reference gathers the witness on the
 * host, relation/src/constraint_system.rs:1225-1247).  mzk_stream_wait_stream(waiter, signaller): work enqueued on `waiter` after
 * this call starts once everything enqueued on `signaller` BEFORE this call has completed (NULL = the null stream). */
MZK_API int32_t mzk_stream_create(void** out_stream);
MZK_API int32_t mzk_stream_destroy(void* stream);
MZK_API int32_t mzk_stream_sync(void* stream);
MZK_API int32_t mzk_stream_wait_stream(void* waiter, void* signaller);
MZK_API int32_t mzk_dev_upload_async(void* dptr, const void* host, uint64_t bytes, void* stream);
MZK_API int32_t mzk_dev_download_async(void* host, const void* dptr, uint64_t bytes, void* stream);
/* device-to-device copy, 2-D copy (pitches and width in bytes) and byte fill, asynchronous on `stream`: what a host
 * orchestrating device-resident rounds needs between kernels (mpc-jellyfish_amd/host/mzk_host.hpp). */
MZK_API int32_t mzk_dev_copy(void* dst, const void* src, uint64_t bytes, void* stream);
/* bytes from device `src_device` to device `dst_device` (logical indices, both initialised), asynchronous on `stream`, a stream of
 * the SOURCE device (NULL = its null stream): hipMemcpyPeerAsync -- over xGMI when the devices can access each other, which
 * mzk_init enables -- or a plain device-to-device copy when both are virtual devices of one card.  The one exchange of a
 * multi-GPU proof (class remainders of the quotient) goes through here. */
MZK_API int32_t mzk_dev_copy_peer(void* dst, int32_t dst_device, const void* src, int32_t src_device, uint64_t bytes, void* stream);
MZK_API int32_t mzk_dev_copy2d(void* dst, uint64_t dst_pitch, const void* src, uint64_t src_pitch, uint64_t width, uint64_t height, void* stream);
MZK_API int32_t mzk_dev_memset(void* dptr, int32_t value, uint64_t bytes, void* stream);
/* `height` runs of `width` bytes, `pitch` bytes apart, in one launch (the tails of the rows of a coefficient slab) */
MZK_API int32_t mzk_dev_memset2d(void* dptr, uint64_t pitch, int32_t value, uint64_t width, uint64_t height, void* stream);

/* ---- measurement hooks (bench.py): HIP-event timing of the library's own kernels ---- */
/* on != 0: every subsequent call brackets its dominant kernels with hipEvents on the launch stream. */
MZK_API int32_t mzk_profile_enable(int32_t on);
/* name: "msm_accumulate", "msm_total", "ntt_pass", "ntt_total", "vfy_transcript" (stage B of mzk_verifier_batch_begin and
 * mzk_verifier_aggregate_begin, either transcript kind), "vfy_link_transcript", "vfy_link_vanishing" (the two kernels of mzk_verifier_link_begin); read the
 * verifier's regions on the device the verifier lives on.  Returns accumulated device
 * milliseconds and launch count since the last reset (synchronises the recorded events). */
MZK_API int32_t mzk_profile_get(const char* name, double* out_ms, uint64_t* out_count);
MZK_API int32_t mzk_profile_reset(void);
/* MSMs of >= 2^17 pairs over a BLS12-381 SRS use a table of precomputed multiples 2^(c*w) * P_i built in HBM on
 * the first such call (13 x the SRS size for 2^20 points); on != 0 (default) enables it.  Results are identical. */
MZK_API int32_t mzk_msm_set_precompute(int32_t on);
/* Builds the table of precomputed multiples of an SRS now (instead of lazily on its first MSM of >= 1024 pairs) and reports it:
 * window bits c, levels W = ceil(256 / c), bytes of HBM it occupies (W x n x 112 B for BLS12-381, x 72 B for BN254: 2 x 9 words of 29-bit limbs) and the wall
 * time the build took (W - 1 launches of c doublings per point, synchronised).  A fixed-base table is legitimate for KZG -- the
 * commit key never changes (primitives/src/pcs/univariate_kzg/srs.rs:77-93) -- but it is a set-up cost ark-ec's
 * VariableBaseMSM does not pay: bench.py prints it beside the headline.  All zeros when the table is disabled or did not fit:
 * a table is only built while it takes at most half of the free HBM, and never beyond MZK_MSM_TABLE_BUDGET bytes (environment; unset = no
 * budget) -- such an SRS commits on the plain (variable-base) path, same points. */
MZK_API int32_t mzk_srs_precompute(uint64_t srs_handle, uint32_t* out_window_bits, uint32_t* out_levels, uint64_t* out_table_bytes,
                                   double* out_build_ms);
/* HBM accounting (bench.py reports it per leg).  An SRS: its points (boundary form + the MSM's internal form: 96 + 112 B per point on
 * BLS12-381, 64 + 72 B on BN254) and its tables: the fixed-base table and the transformed SRS vector of mzk_kzg_multi_open_rou_dev (0 until
 * built; the reference keeps the points only: srs.rs:36-40).  A proving
 * key: the resident evaluations of the fixed polynomials and the per-point tables.  The device context: the shared scratch of the NTT /
 * MSM / quotient kernels (grow-only) and the buffers of the host-pointer I/O slots. */
MZK_API int32_t mzk_srs_hbm_bytes(uint64_t srs_handle, uint64_t* out_points_bytes, uint64_t* out_table_bytes);
MZK_API int32_t mzk_plonk_pk_hbm_bytes(uint64_t pk_handle, uint64_t* out_bytes);
MZK_API int32_t mzk_workspace_hbm_bytes(uint64_t* out_bytes);
/* Frees that scratch (synchronises the device; it grows again on demand). */
MZK_API int32_t mzk_workspace_release(void);
/* Kernel launches the library has made in this process so far (all device contexts; copies and fills are not kernels): bench.py
 * reports launches per proof and per MSM from differences of it.  out may not be null. */
MZK_API int32_t mzk_launch_count(uint64_t* out_launches);
/* Last MSM's shape: window bits, windows, buckets per window (for DESIGN.md's op counts). */
MZK_API int32_t mzk_msm_last_shape(uint32_t* out_window_bits, uint32_t* out_windows, uint32_t* out_buckets);
/* Rare-path sizing of the calling context's last MSM group: per-thread run cap, chunk-descriptor capacity and level-1 capacity per
 * bucket set of its last MSM, and how many times the group ran (1 = no overflow).  For tests. */
MZK_API int32_t mzk_msm_last_rare(uint32_t* out_cap, uint32_t* out_desc_cap, uint32_t* out_h1_cap, uint32_t* out_attempts);

#ifdef __cplusplus
}
#endif
#endif /* MZK_H */
