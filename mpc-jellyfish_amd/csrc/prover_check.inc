// prover_check.inc -- mzk_prover_check_witness: where a witness fails (Circuit::check_circuit_satisfiability, constraint_system.rs:389-451).
// Member function of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ).  No kernels here:
// the arguments are validated as round 1 validates them and the three families run on the proving key's device (plonk.hip
// witness_check_run, check.cuh) on the handle's stream S, in the context's shared scratch -- the handle allocates nothing.

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::check_witness(int kind, const void* witness, uint64_t witness_len, const uint64_t* pi_rows, const uint64_t* pi, uint64_t n_pi,
        mzk_witness_report* out) {
    if (!out || !witness || (n_pi && !pi)) fail(MZK_ERR_INVALID_ARG, "null pointer");
    const bool vec = kind == MZK_WITNESS_HOST_VECTOR || kind == MZK_WITNESS_DEV_VECTOR;
    if (!vec && kind != MZK_WITNESS_DEV_WIRES && kind != MZK_WITNESS_HOST_WIRES) fail(MZK_ERR_INVALID_ARG, "unknown witness_kind");
    if (vec && !vars_dev()) fail(MZK_ERR_INVALID_ARG, "mzk_prover_set_wire_variables has not been called");
    if (vec ? witness_len != vars_n() : witness_len != (uint64_t)W * n)
        fail(MZK_ERR_INVALID_ARG, vec ? "witness_len != the n_vars of mzk_prover_set_wire_variables" : "witness_len != num_wire_types * domain size");
    if (!pi_rows && n_pi > n) fail(MZK_ERR_INVALID_ARG, "more public inputs than rows");
    for (uint64_t i = 0; pi_rows && i < n_pi; i++)
        if (pi_rows[i] >= n) fail(MZK_ERR_INVALID_ARG, "public-input row outside the domain");
    // a proof in flight is abandoned, as by a new round 1: the next round call must be round 1
    st = State();
    stage = CREATED;
    if (S) ck(mzk_stream_wait_stream(S, nullptr));                 // a device-resident witness written on the null stream is complete first
    WitnessCheckIn in{};
    in.d_sel_coeffs = static_cast<const uint32_t*>(fix(0));
    in.kind = kind;
    in.witness = witness;
    in.d_vars = static_cast<const uint32_t*>(vars_dev());
    in.n_vars = vars_n();
    in.pi_rows = pi_rows; in.pi = pi; in.n_pi = n_pi;
    ck(mzk_ctx_check_witness(key().pk, &in, out, S));
}
