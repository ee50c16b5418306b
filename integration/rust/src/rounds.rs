//! Round-level swap: the BODIES of `Prover::run_1st_round .. compute_opening_proofs`
//! (plonk/src/proof_system/prover.rs:72-419) replaced by `mzk_prover_round1 .. round5` (include/mzk.h; csrc/prover.hip).
//! `batch_prove_internal` (plonk/src/proof_system/snark.rs:201-469) keeps its shape: the same loops over the instances, the same
//! transcript calls between the rounds, the same `prng` draws in the same order -- so `PlonkKzgSnark::prove`'s signature and the
//! proof bytes are unchanged.  What changes is where the polynomials live: `Oracles` (structs.rs:875-887) is replaced by one
//! `Mi355Prover` per instance whose vectors stay in HBM from the wire iNTTs to the opening MSMs.
//!
//! This file is meant to live in the reference's `plonk` crate as `src/proof_system/mi355_rounds.rs` behind
//! `#[cfg(feature = "mi355")]`; it needs one accessor added to `relation` (the fields are `pub(crate)` there,
//! relation/src/constraint_system.rs:127, 131):
//!     impl<F: FftField> PlonkCircuit<F> { pub fn witness_and_wire_variables(&self) -> (&[F], &[Vec<Variable>; GATE_WIDTH + 2]) }
//! NOT COMPILED in this repository's image (no Rust toolchain); the C++ host (mpc-jellyfish_amd/host/mzk_prover.hpp) and the ctypes
//! driver (mpc-jellyfish_amd/prover.py) are the compiled / executed twins of exactly this call sequence.
use ark_ec::{pairing::Pairing, short_weierstrass::Affine, AffineRepr};
use ark_ff::{PrimeField, UniformRand};
use ark_std::rand::{CryptoRng, RngCore};
use core::ffi::c_void;
use std::sync::Arc;

use ark_serialize::CanonicalSerialize;

use crate::{check, mzk_prover_create_serialized, mzk_prover_serialize_key, mzk_prover_serialize_vk, mzk_srs_release, Mi355Error, SrsHandle, MZK_ERR_ENCODING,
            MZK_KEY_CHECK_COMMITMENTS, MZK_SER_COMPRESSED, MZK_SER_VALIDATE};

pub const MZK_WITNESS_HOST_VECTOR: i32 = 2;
pub const MZK_ERR_WRONG_QUOTIENT_DEGREE: i32 = -9;
pub const MZK_CHECK_SATISFIED: u32 = 0;
pub const MZK_CHECK_GATE: u32 = 1;
pub const MZK_CHECK_LOOKUP: u32 = 2;
pub const MZK_CHECK_COPY: u32 = 3;

/// `mzk_witness_report` (include/mzk.h): where a witness fails -- the first failing family in the order gate, lookup, copy, the number
/// of failing gate rows / lookup rows / copy cells and the lowest of each (`u64::MAX` = none; cells as `wire * n + row`), the W wire
/// values of the reported row and, for the gate family, the residual of the gate identity on it (Montgomery limbs).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct WitnessReport {
    pub kind: u32,
    pub copy_checked: u32,
    pub gate_failures: u64,
    pub gate_row: u64,
    pub lookup_failures: u64,
    pub lookup_row: u64,
    pub copy_failures: u64,
    pub copy_cell: u64,
    pub copy_rep_cell: u64,
    pub row_wires: [u64; 24],
    pub gate_residual: [u64; 4],
}

impl WitnessReport {
    pub fn satisfied(&self) -> bool {
        self.kind == MZK_CHECK_SATISFIED
    }
}

#[cfg_attr(feature = "link", link(name = "mi355zk"))]
extern "C" {
    pub fn mzk_srs_lagrange_from_srs(srs: u64, log_n: u32, n_extra: u32, out_handle: *mut u64) -> i32;
    pub fn mzk_prover_create(curve_id: i32, log_n: u32, num_wire_types: u32, selector_coeffs: *const u64, sigma_coeffs: *const u64,
                             table_coeffs: *const u64, poly_len: u64, k_mont: *const u64, commit_key: u64, lagrange_key: u64,
                             comm: *const c_void, out_prover: *mut u64) -> i32;
    pub fn mzk_prover_create_from_circuit(curve_id: i32, log_n: u32, num_wire_types: u32, selector_values: *const u64, wire_variables: *const u32,
                                          n_vars: u64, table_values: *const u64, k_mont: *const u64, commit_key: u64, lagrange_key: u64,
                                          comm: *const c_void, out_prover: *mut u64) -> i32;
    pub fn mzk_prover_destroy(prover: u64) -> i32;
    pub fn mzk_prover_fork(prover: u64, out_prover: *mut u64) -> i32;
    pub fn mzk_prover_hbm_bytes(prover: u64, out_fixed: *mut u64, out_proving_key: *mut u64, out_workspace: *mut u64) -> i32;
    pub fn mzk_prover_shared_hbm_bytes(prover: u64, out_shared_bytes: *mut u64, out_sharers: *mut u32) -> i32;
    pub fn mzk_prover_set_wire_variables(prover: u64, wire_variables: *const u32, n_vars: u64) -> i32;
    // the same table recovered from the key's sigma polynomials (a `ProvingKey` does not carry `wire_variables`), and its download;
    // the two stateless steps underneath, on device arrays
    pub fn mzk_prover_derive_wire_variables(prover: u64, out_n_vars: *mut u64) -> i32;
    pub fn mzk_prover_get_wire_variables(prover: u64, out_wire_variables: *mut u32, capacity_cells: u64, out_n_vars: *mut u64) -> i32;
    pub fn mzk_plonk_sigma_decode_dev(curve_id: i32, log_n: u32, num_wire_types: u32, d_sigma_values: *const c_void, k_mont: *const u64,
                                      d_out_next_u32: *mut c_void, stream: *mut c_void) -> i32;
    pub fn mzk_plonk_variables_from_permutation_dev(d_next_u32: *const c_void, cells: u64, d_out_variables_u32: *mut c_void, out_n_vars: *mut u64,
                                                    stream: *mut c_void) -> i32;
    pub fn mzk_prover_round1(prover: u64, witness_kind: i32, witness: *const c_void, witness_len: u64, pub_input_rows: *const u64,
                             pub_input_mont: *const u64, n_pub: u64, blinders_mont: *const u64, out_comms_xy: *mut u64) -> i32;
    pub fn mzk_prover_check_witness(prover: u64, witness_kind: i32, witness: *const c_void, witness_len: u64, pub_input_rows: *const u64,
                                    pub_input_mont: *const u64, n_pub: u64, out_report: *mut WitnessReport) -> i32;
    pub fn mzk_prover_round1_5(prover: u64, tau: *const u64, blinders: *const u64, out_comms_xy: *mut u64) -> i32;
    pub fn mzk_prover_round2(prover: u64, beta: *const u64, gamma: *const u64, blinders: *const u64, out_comm_xy: *mut u64) -> i32;
    pub fn mzk_prover_round2_5(prover: u64, blinders: *const u64, out_comm_xy: *mut u64) -> i32;
    pub fn mzk_prover_round3(provers: *const u64, n_instances: u32, alpha: *const u64, blinders: *const u64, out_comms_xy: *mut u64) -> i32;
    pub fn mzk_prover_round4(prover: u64, zeta: *const u64, out_evals: *mut u64) -> i32;
    pub fn mzk_prover_round5(provers: *const u64, n_instances: u32, v: *const u64, out_comms_xy: *mut u64) -> i32;
}

/// A Lagrange-basis key derived for a prover: its points and fixed-base table live in HBM until the last slot that uses it is dropped.
struct LagrangeKey(u64);

impl Drop for LagrangeKey {
    fn drop(&mut self) {
        unsafe {
            mzk_srs_release(self.0);
        }
    }
}

/// One instance's device-resident state: `ProvingKey{selectors, sigmas, plookup_pk}` (structs.rs:575-590) uploaded once, the
/// circuit's wire-variable table, and the workspace of the proof in flight.  Created once per proving key; `fork` makes the further
/// instance slots on the same key.
pub struct Mi355Prover {
    pub handle: u64,
    pub num_wire_types: usize,
    pub ultra: bool,
    fq_limbs: usize,
    /// the Lagrange-basis key derived for this prover (None = round 1 commits the coefficient forms), shared with its forks
    lagrange_key: Option<Arc<LagrangeKey>>,
    /// the commit key registered from a serialized `ProvingKey` (`from_proving_key`; None = the caller's `SrsHandle`), shared with its forks
    embedded_commit_key: Option<Arc<LagrangeKey>>,
}

impl Drop for Mi355Prover {
    fn drop(&mut self) {
        unsafe {
            mzk_prover_destroy(self.handle); // (the Lagrange key goes after it, with the last slot: fields drop after this body)
        }
    }
}

fn owned(lagrange: u64) -> Option<Arc<LagrangeKey>> {
    if lagrange != 0 { Some(Arc::new(LagrangeKey(lagrange))) } else { None }
}

fn flat<F: PrimeField>(v: &[F]) -> *const u64 {
    v.as_ptr() as *const u64 // Fp<MontBackend<_, 4>, 4> is a [u64; 4] newtype in Montgomery form: the byte image the ABI takes
}

impl Mi355Prover {
    /// `selectors` / `sigmas` / `tables`: the coefficient vectors of the proving key's polynomials, each padded to n = 2^log_n and
    /// concatenated (what `pk.selectors.iter().flat_map(|p| padded(p.coeffs()))` yields); `commit_key`: the registered
    /// `pk.commit_key.powers_of_g` (n + 3 points); `wire_variables`: W x n variable indices, wire-major.
    #[allow(clippy::too_many_arguments)]
    pub fn new<F: PrimeField>(curve_id: i32, log_n: u32, selectors: &[F], sigmas: &[F], tables: Option<&[F]>, k: &[F], commit_key: &SrsHandle,
                              lagrange_round1: bool, wire_variables: &[u32], n_vars: usize, fq_limbs: usize) -> Result<Self, Mi355Error> {
        let num_wire_types = k.len();
        let (mut lagrange, mut handle) = (0u64, 0u64);
        unsafe {
            if lagrange_round1 {
                // [L_i(beta)]g from the SRS's own points (inverse NTT over the group, once per SRS and domain): round 1 then commits the
                // wire VALUES -- same group elements, mostly small scalars
                check(mzk_srs_lagrange_from_srs(commit_key.raw(), log_n, 3, &mut lagrange))?;
            }
            let made = check(mzk_prover_create(curve_id, log_n, num_wire_types as u32, flat(selectors), flat(sigmas),
                                               tables.map_or(core::ptr::null(), |t| flat(t)), 1u64 << log_n, flat(k), commit_key.raw(), lagrange,
                                               core::ptr::null(), &mut handle));
            if made.is_err() && lagrange != 0 {
                mzk_srs_release(lagrange);                         // nothing of a failed construction stays in HBM
            }
            made?;
        }
        // from here on Drop releases both handles
        let me = Self { handle, num_wire_types, ultra: tables.is_some(), fq_limbs, lagrange_key: owned(lagrange), embedded_commit_key: None };
        unsafe { check(mzk_prover_set_wire_variables(handle, wire_variables.as_ptr(), n_vars as u64))? };
        Ok(me)
    }

    /// The same prover from the FINALISED CIRCUIT instead of a `ProvingKey`: `PlonkKzgSnark::preprocess` (snark.rs:529-617) on the
    /// device.  `selector_values` / `table_values`: the VALUES on the gate domain, each vector of length n = 2^log_n, concatenated
    /// (`cs.all_selectors()` before `compute_selector_polynomials`' iFFTs, constraint_system.rs:1162-1177; range, key, table_dom_sep,
    /// q_dom_sep); `wire_variables`: W x n variable indices, wire-major.  compute_wire_permutation, compute_extended_permutation and
    /// the 13 + W (+ 4) iFFTs run inside the library; nothing but nsel x n x 32 B of selector values and W x n x 4 B of indices is
    /// uploaded, and no CPU preprocess is needed.  The variable table stays with the prover: no `mzk_prover_set_wire_variables`.
    #[allow(clippy::too_many_arguments)]
    pub fn from_circuit<F: PrimeField>(curve_id: i32, log_n: u32, selector_values: &[F], table_values: Option<&[F]>, k: &[F], commit_key: &SrsHandle,
                                       lagrange_round1: bool, wire_variables: &[u32], n_vars: usize, fq_limbs: usize) -> Result<Self, Mi355Error> {
        let num_wire_types = k.len();
        let (mut lagrange, mut handle) = (0u64, 0u64);
        unsafe {
            if lagrange_round1 {
                check(mzk_srs_lagrange_from_srs(commit_key.raw(), log_n, 3, &mut lagrange))?;
            }
            let made = check(mzk_prover_create_from_circuit(curve_id, log_n, num_wire_types as u32, flat(selector_values), wire_variables.as_ptr(),
                                                            n_vars as u64, table_values.map_or(core::ptr::null(), |t| flat(t)), flat(k),
                                                            commit_key.raw(), lagrange, core::ptr::null(), &mut handle));
            if made.is_err() && lagrange != 0 {
                mzk_srs_release(lagrange);                         // nothing of a failed construction stays in HBM
            }
            made?;
        }
        Ok(Self { handle, num_wire_types, ultra: table_values.is_some(), fq_limbs, lagrange_key: owned(lagrange), embedded_commit_key: None })
    }

    /// The same prover from a `ProvingKey<E>` as it is: `pk.serialize_compressed()` (ark-serialize 0.4; the image every Rust deployment
    /// already writes next to its SRS) handed to `mzk_prover_create_serialized`, which parses the container on the host and decodes the
    /// polynomials, `k` and the commit key on the device -- no field element is pulled apart on the Rust side.  `commit_key`: a registered
    /// SRS to use instead of the embedded one (one SRS and its fixed-base table then serve many keys; the embedded points are skipped, not
    /// compared); `check_commitments`: the commitments in `pk.vk` must commit the key's polynomials (`MZK_KEY_CHECK_COMMITMENTS`).  The
    /// prover has no wire-variable table: `mzk_prover_derive_wire_variables` recovers one from sigma, or set the circuit's.
    /// Parity of the library's restatement of the format with ark's derive is UNPINNED until `gen_fixtures proving_key` has been run
    /// (tests/golden/ref_proving_keys.json).
    pub fn from_proving_key<K: CanonicalSerialize>(curve_id: i32, pk: &K, num_wire_types: usize, commit_key: Option<&SrsHandle>, lagrange_round1: bool,
                                                   check_commitments: bool, fq_limbs: usize) -> Result<Self, Mi355Error> {
        let mut bytes = Vec::with_capacity(pk.compressed_size());
        pk.serialize_compressed(&mut bytes).map_err(|e| Mi355Error(MZK_ERR_ENCODING, e.to_string()))?;
        let flags = MZK_SER_COMPRESSED | MZK_SER_VALIDATE | if check_commitments { MZK_KEY_CHECK_COMMITMENTS } else { 0 };
        let (mut handle, mut ck, mut lagrange, mut bad) = (0u64, 0u64, 0u64, 0u64);
        unsafe {
            check(mzk_prover_create_serialized(curve_id, bytes.as_ptr(), bytes.len() as u64, flags, commit_key.map_or(0, |s| s.raw()), core::ptr::null(),
                                               &mut handle, &mut ck, if lagrange_round1 { &mut lagrange } else { core::ptr::null_mut() }, &mut bad))?;
        }
        Ok(Self { handle, num_wire_types, ultra: num_wire_types == 6, fq_limbs, lagrange_key: owned(lagrange), embedded_commit_key: owned(ck) })
    }

    /// `CanonicalSerialize` of the `ProvingKey` (or, `vk_only`, the `VerifyingKey`) of this prover, however it was created -- a key
    /// preprocessed on the device goes back to Rust as bytes `ProvingKey::<E>::deserialize_compressed` reads.  `h` / `beta_h`: the open
    /// key's G2 elements serialized in the same mode (the library does not hold them).
    pub fn serialize_key(&self, vk_only: bool, compressed: bool, num_inputs: usize, h: &[u8], beta_h: &[u8], is_merged: bool) -> Result<Vec<u8>, Mi355Error> {
        let f = if vk_only { mzk_prover_serialize_vk } else { mzk_prover_serialize_key };
        let flags = if compressed { MZK_SER_COMPRESSED } else { 0 };
        let mut len = 0u64;
        unsafe { check(f(self.handle, flags, num_inputs as u64, core::ptr::null(), core::ptr::null(), is_merged as i32, core::ptr::null_mut(), 0, &mut len))? };
        let mut out = vec![0u8; len as usize];
        unsafe { check(f(self.handle, flags, num_inputs as u64, h.as_ptr(), beta_h.as_ptr(), is_merged as i32, out.as_mut_ptr(), len, &mut len))? };
        Ok(out)
    }

    /// Another slot on this prover's proving key (`mzk_prover_fork`): the key, its Lagrange key and the variable table stay ONE copy in
    /// HBM, the slot brings its own workspace and stream.  `batch_prove(&[&circuit; K], &[&pk; K])` -- one `ProvingKey` K times,
    /// snark.rs:64-78 -- becomes `prove_rounds` over the prover and K - 1 forks of it; the same slots serve K proofs in flight from K
    /// threads.  Slots are peers and drop in any order.  No SRS work, no NTT, no upload.
    pub fn fork(&self) -> Result<Self, Mi355Error> {
        let mut handle = 0u64;
        unsafe { check(mzk_prover_fork(self.handle, &mut handle))? };
        Ok(Self { handle, num_wire_types: self.num_wire_types, ultra: self.ultra, fq_limbs: self.fq_limbs, lagrange_key: self.lagrange_key.clone(),
                  embedded_commit_key: self.embedded_commit_key.clone() })
    }

    /// (fixed coefficient forms, proving-key evaluations, workspace) this slot reaches, then the bytes among them that other living
    /// slots reach too and the number of slots on the key: K slots hold sum(fixed + key + workspace) - (K - 1) * shared.
    pub fn hbm_bytes(&self) -> Result<(u64, u64, u64, u64, u32), Mi355Error> {
        let (mut fixed, mut key, mut ws, mut shared, mut sharers) = (0u64, 0u64, 0u64, 0u64, 0u32);
        unsafe {
            check(mzk_prover_hbm_bytes(self.handle, &mut fixed, &mut key, &mut ws))?;
            check(mzk_prover_shared_hbm_bytes(self.handle, &mut shared, &mut sharers))?;
        }
        Ok((fixed, key, ws, shared, sharers))
    }

    /// `Circuit::check_circuit_satisfiability` (relation/src/constraint_system.rs:389-451) on the device, for the witness vector
    /// `prove_rounds` hands to round 1 (`cs.witness_and_wire_variables().0`) and the public input on rows 0 .. : which gate row or
    /// lookup row fails first and how many do.  Copy constraints hold by construction for a witness vector.  A proof in flight on
    /// this prover is abandoned.
    pub fn check_witness<F: PrimeField>(&self, witness: &[F], pub_input: &[F]) -> Result<WitnessReport, Mi355Error> {
        let mut report = WitnessReport::default();
        unsafe {
            check(mzk_prover_check_witness(self.handle, MZK_WITNESS_HOST_VECTOR, witness.as_ptr() as *const c_void, witness.len() as u64,
                                           core::ptr::null(), flat(pub_input), pub_input.len() as u64, &mut report))?;
        }
        Ok(report)
    }

    fn points<P: ark_ec::short_weierstrass::SWCurveConfig>(&self, xy: &[u64]) -> Vec<Affine<P>>
    where P::BaseField: PrimeField {
        xy.chunks(2 * self.fq_limbs).map(|c| crate::affine_from_limbs::<P>(c)).collect() // (0, 0) = infinity
    }
}

/// `DensePolynomial::rand(hiding_bound, prng)` draws hiding_bound + 1 coefficients, low order first (ark-poly): these ARE the
/// blinders b_0 .. b_h of `mask_polynomial` (prover.rs:463-486): p + (b_0 + b_1 X + ..)(X^n - 1).
fn draw<F: PrimeField, R: RngCore + CryptoRng>(prng: &mut R, count: usize) -> Vec<F> {
    (0..count).map(|_| F::rand(prng)).collect()
}

/// The round calls of `batch_prove_internal` (snark.rs:263-431) with the device prover.  `T`, `E`, `circuits`, `prove_keys`,
/// `transcript`, `challenges` as in the reference; `provers[i]` belongs to `(prove_keys[i], circuits[i])`.
/// Returns what the reference assembles into `BatchProof` (snark.rs:453-462).
#[cfg(feature = "reference-types")]
pub fn prove_rounds<E, F, P, C, R, T>(prng: &mut R, circuits: &[&C], provers: &[&Mi355Prover], transcript: &mut T)
    -> Result<BatchProof<E>, PlonkError>
where
    E: Pairing<BaseField = F, G1Affine = Affine<P>>, F: RescueParameter + SWToTEConParam, P: SWCurveConfig<BaseField = F>,
    C: Arithmetization<E::ScalarField>, R: CryptoRng + RngCore, T: PlonkTranscript<F>,
{
    let w = provers[0].num_wire_types;
    let ql = provers[0].fq_limbs;
    let handles: Vec<u64> = provers.iter().map(|p| p.handle).collect();
    let fail = |rc: i32| -> PlonkError {
        if rc == MZK_ERR_WRONG_QUOTIENT_DEGREE { SnarkError::WrongQuotientPolyDegree(0, 0).into() } else { SnarkError::ParameterError(crate::last_error()).into() }
    };
    // Round 1 (prover.rs:72-87): the witness vector crosses PCIe once; gather, iNTTs, masking, batch_commit on the device
    let mut wires_poly_comms_vec = vec![];
    for (cs, p) in circuits.iter().zip(provers) {
        let (witness, _) = cs.witness_and_wire_variables();
        let pub_input = cs.public_input()?;                       // rows 0 .. num_inputs - 1 after finalize_for_arithmetization
        let blinders: Vec<E::ScalarField> = draw(prng, 2 * w);    // W x DensePolynomial::rand(1), in wire order
        let mut xy = vec![0u64; w * 2 * ql];
        let rc = unsafe { mzk_prover_round1(p.handle, MZK_WITNESS_HOST_VECTOR, witness.as_ptr() as *const c_void, witness.len() as u64,
                                            core::ptr::null(), flat(&pub_input), pub_input.len() as u64, flat(&blinders), xy.as_mut_ptr()) };
        if rc != 0 { return Err(fail(rc)); }
        let comms: Vec<Commitment<E>> = p.points::<P>(&xy).into_iter().map(Commitment).collect();
        transcript.append_commitments(b"witness_poly_comms", &comms)?;
        wires_poly_comms_vec.push(comms);
    }
    // Round 1.5 (prover.rs:89-118)
    let tau = transcript.get_and_append_challenge::<E>(b"tau")?;
    let mut h_poly_comms_vec = vec![];
    for p in provers {
        h_poly_comms_vec.push(if p.ultra {
            let blinders: Vec<E::ScalarField> = draw(prng, 6);    // h_1, h_2: DensePolynomial::rand(2) each
            let mut xy = vec![0u64; 2 * 2 * ql];
            let rc = unsafe { mzk_prover_round1_5(p.handle, flat(&[tau]), flat(&blinders), xy.as_mut_ptr()) };
            if rc != 0 { return Err(fail(rc)); }
            let comms: Vec<Commitment<E>> = p.points::<P>(&xy).into_iter().map(Commitment).collect();
            transcript.append_commitments(b"h_poly_comms", &comms)?;
            Some(comms)
        } else { None });
    }
    // Round 2 (prover.rs:125-141)
    let beta = transcript.get_and_append_challenge::<E>(b"beta")?;
    let gamma = transcript.get_and_append_challenge::<E>(b"gamma")?;
    let mut prod_perm_poly_comms_vec = vec![];
    for p in provers {
        let blinders: Vec<E::ScalarField> = draw(prng, 3);
        let mut xy = vec![0u64; 2 * ql];
        let rc = unsafe { mzk_prover_round2(p.handle, flat(&[beta]), flat(&[gamma]), flat(&blinders), xy.as_mut_ptr()) };
        if rc != 0 { return Err(fail(rc)); }
        let comm = Commitment(p.points::<P>(&xy)[0]);
        transcript.append_commitment(b"perm_poly_comms", &comm)?;
        prod_perm_poly_comms_vec.push(comm);
    }
    // Round 2.5 (prover.rs:143-183)
    let mut prod_lookup_poly_comms_vec = vec![];
    for p in provers {
        prod_lookup_poly_comms_vec.push(if p.ultra {
            let blinders: Vec<E::ScalarField> = draw(prng, 3);
            let mut xy = vec![0u64; 2 * ql];
            let rc = unsafe { mzk_prover_round2_5(p.handle, flat(&blinders), xy.as_mut_ptr()) };
            if rc != 0 { return Err(fail(rc)); }
            let comm = Commitment(p.points::<P>(&xy)[0]);
            transcript.append_commitment(b"plookup_poly_comms", &comm)?;
            Some(comm)
        } else { None });
    }
    // Round 3 (prover.rs:192-209): ONE call over all instances -- quotient, split (W - 1 draws), W commitments
    let alpha = transcript.get_and_append_challenge::<E>(b"alpha")?;
    let blinders: Vec<E::ScalarField> = draw(prng, w - 1);
    let mut xy = vec![0u64; w * 2 * ql];
    let rc = unsafe { mzk_prover_round3(handles.as_ptr(), handles.len() as u32, flat(&[alpha]), flat(&blinders), xy.as_mut_ptr()) };
    if rc != 0 { return Err(fail(rc)); }
    let split_quot_poly_comms: Vec<Commitment<E>> = provers[0].points::<P>(&xy).into_iter().map(Commitment).collect();
    transcript.append_commitments(b"quot_poly_comms", &split_quot_poly_comms)?;
    // Rounds 4 / 4.5 (prover.rs:216-299): ProofEvaluations of every instance first, then the PlookupEvaluations (snark.rs:365-399)
    let zeta = transcript.get_and_append_challenge::<E>(b"zeta")?;
    let (mut poly_evals_vec, mut plookup_evals_vec) = (vec![], vec![]);
    for p in provers {
        let mut ev = vec![E::ScalarField::zero(); 2 * w + if p.ultra { 15 } else { 0 }];
        let rc = unsafe { mzk_prover_round4(p.handle, flat(&[zeta]), ev.as_mut_ptr() as *mut u64) };
        if rc != 0 { return Err(fail(rc)); }
        let poly_evals = ProofEvaluations { wires_evals: ev[..w].to_vec(), wire_sigma_evals: ev[w..2 * w - 1].to_vec(), perm_next_eval: ev[2 * w - 1] };
        transcript.append_proof_evaluations::<E>(&poly_evals)?;
        poly_evals_vec.push(poly_evals);
        plookup_evals_vec.push(if p.ultra { Some(plookup_evaluations_from_slice(&ev[2 * w..])) } else { None });   // declaration order, structs.rs:496-541
    }
    for evals in plookup_evals_vec.iter().flatten() {
        transcript.append_plookup_evaluations::<E>(evals)?;
    }
    // Round 5 (prover.rs:302-460): linearisation polynomial and both opening proofs, ONE call.  MZK_ERR_WRONG_QUOTIENT_DEGREE here
    // is the quotient identity failing at zeta: the witness does not satisfy the circuit (the reference raises it in round 3)
    let v = transcript.get_and_append_challenge::<E>(b"v")?;
    let mut xy = vec![0u64; 2 * 2 * ql];
    let rc = unsafe { mzk_prover_round5(handles.as_ptr(), handles.len() as u32, flat(&[v]), xy.as_mut_ptr()) };
    if rc != 0 { return Err(fail(rc)); }
    let open = provers[0].points::<P>(&xy);
    let plookup_proofs_vec = (0..provers.len()).map(|i| plookup_evals_vec[i].clone().map(|poly_evals| PlookupProof {
        h_poly_comms: h_poly_comms_vec[i].clone().unwrap(), prod_lookup_poly_comm: prod_lookup_poly_comms_vec[i].unwrap(), poly_evals })).collect();
    Ok(BatchProof { wires_poly_comms_vec, prod_perm_poly_comms_vec, poly_evals_vec, plookup_proofs_vec, split_quot_poly_comms,
                    opening_proof: Commitment(open[0]), shifted_opening_proof: Commitment(open[1]) })
}
