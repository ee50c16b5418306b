"""GPU: serialized ProvingKey / VerifyingKey images (include/mzk.h: mzk_fr_decode_dev / mzk_fr_encode_dev, mzk_prover_create_serialized,
mzk_prover_serialize_key / _vk; mpc-jellyfish_amd/keys.py).  Every image is made on the test side from oracle integers (tests/keyimg.py):
coefficient forms by the oracle's big-int inverse NTT with trailing zeros stripped, the commit key beta^i g, the commitments those the
golden vectors hold.  Parity of the format itself with the Rust code is unpinned until tests/golden/ref_proving_keys.json exists."""
import ctypes as C
import json
import os
import random
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import check_witness_ref as REF
import keyimg
from conftest import fr_mont_limbs, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ENCODING = -11
TABLES = ("range", "key", "table_dom_sep", "q_dom_sep")


# ---- Fr primitives ---------------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 255, 256, 257, 1000)
ROW_LEN = 1024                                                     # longer than every count (the tail must read zero), four blocks of 256


@lru_cache(maxsize=None)
def _fr_values(curve_id):
    """1000 values -- 0, 1, r - 1 first, seeded random after -- their 32-byte records and their Montgomery limbs (big-int arithmetic here)"""
    import pyref
    pc = pyref.CURVES[curve_id]
    rnd = random.Random(4100 + curve_id)
    vals = [0, 1, pc.r - 1] + [rnd.randrange(pc.r) for _ in range(max(COUNTS) - 3)]
    return vals, b"".join(v.to_bytes(32, "little") for v in vals), fr_mont_limbs(pc, vals)


def _decode(gpu, curve_id, image: bytes, segs, n_rows, row_len):
    """mzk_fr_decode_dev on torch memory: segs = [(offset, count, row)].  Returns (rc, bad segment, bad index, rows as uint64 numpy)."""
    import torch
    L = gpu.load()
    img = torch.frombuffer(bytearray(image + bytes(-len(image) % 4 or 4)), dtype=torch.uint8).cuda()
    out = torch.full((n_rows, row_len, 4), -1, dtype=torch.int64, device="cuda")          # garbage: the zero fill must overwrite it
    src, cnt = (np.array([s[i] for s in segs], dtype=np.uint64) for i in (0, 1))
    row = np.array([s[2] for s in segs], dtype=np.uint32)
    bad_seg, bad_idx = C.c_uint32(), C.c_uint64()
    torch.cuda.synchronize()
    rc = L.mzk_fr_decode_dev(curve_id, C.c_void_p(img.data_ptr()), len(image), len(segs), C.c_void_p(src.ctypes.data), C.c_void_p(cnt.ctypes.data),
                             C.c_void_p(row.ctypes.data), C.c_void_p(out.data_ptr()), n_rows, row_len, C.byref(bad_seg), C.byref(bad_idx), None)
    return rc, bad_seg.value, bad_idx.value, out.cpu().numpy().view(np.uint64), out


@pytest.mark.parametrize("curve_id", [0, 1])
def test_fr_records_decode_at_every_alignment_and_encode_back(gpu, curve_id):
    import torch
    L = gpu.load()
    vals, recs, mont = _fr_values(curve_id)
    for residue in range(8):
        image, segs = bytearray(), []
        for row, count in enumerate(COUNTS):                       # rows in reverse order: a segment's row is its own business
            image += bytes((residue - len(image)) % 8) if row == 0 else bytes(8 + (residue - len(image)) % 8)
            assert len(image) % 8 == residue
            segs.append((len(image), count, len(COUNTS) - 1 - row))
            image += recs[:32 * count]
        rc, bad_seg, bad_idx, rows, dev = _decode(gpu, curve_id, bytes(image), segs, len(COUNTS), ROW_LEN)
        assert rc == 0 and bad_seg == 2**32 - 1 and bad_idx == 2**64 - 1, L.mzk_last_error()
        for off, count, row in segs:
            assert np.array_equal(rows[row, :count], mont[:count]), (residue, count)
            assert not rows[row, count:].any(), (residue, count)
        # encoding a decoded row gives the bytes back
        off, count, row = segs[-1]
        back = torch.zeros(32 * count, dtype=torch.uint8, device="cuda")
        assert L.mzk_fr_encode_dev(curve_id, C.c_void_p(dev[row].data_ptr()), count, C.c_void_p(back.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert bytes(back.cpu().numpy()) == recs[:32 * count]


@pytest.mark.parametrize("curve_id", [0, 1])
def test_fr_records_not_below_the_modulus_are_refused_lowest_first(gpu, curve_id):
    import pyref
    L = gpu.load()
    r = pyref.CURVES[curve_id].r
    vals, recs, _ = _fr_values(curve_id)
    rec = lambda v: v.to_bytes(32, "little")
    for bad_value in (r, r + 1, 2**256 - 1):
        image = bytearray(b"\0" + recs[:32 * 300])
        image[1 + 32 * 299:1 + 32 * 300] = rec(bad_value)
        rc, bad_seg, bad_idx, _, _ = _decode(gpu, curve_id, bytes(image), [(1, 300, 0)], 1, 512)
        assert rc == ERR_ENCODING and (bad_seg, bad_idx) == (0, 299)
        assert L.mzk_last_error().decode() == "segment 0 coefficient 299: not below the modulus"
    # several of them placed: the lowest (segment, index) in segment order, whatever the byte order in the image, the same on two runs
    image = bytearray(3 + 3 * 32 * 700)
    segs = [(3 + 2 * 32 * 700, 700, 0), (3, 700, 1), (3 + 32 * 700, 700, 2)]
    for off, count, _ in segs:
        image[off:off + 32 * count] = recs[:32 * count]
    for seg, idx, v in ((2, 5, r), (1, 699, 2**256 - 1), (1, 257, r + 1), (1, 600, r)):
        image[segs[seg][0] + 32 * idx:segs[seg][0] + 32 * idx + 32] = rec(v)
    for _ in range(2):
        rc, bad_seg, bad_idx, _, _ = _decode(gpu, curve_id, bytes(image), segs, 3, 1024)
        assert rc == ERR_ENCODING and (bad_seg, bad_idx) == (1, 257)
    # arguments that would read or write outside are refused before any launch
    for segs_bad in ([(0, 1025, 0)], [(len(image) - 31, 1, 0)], [(0, 1, 3)]):
        assert _decode(gpu, curve_id, bytes(image), segs_bad, 3, 1024)[0] == -1


# ---- whole keys ------------------------------------------------------------------------------------------------------------------------
def _coeffs(pc, log_n, values):
    """DensePolynomial of the values on the gate domain: the oracle's big-int inverse NTT, trailing zeros stripped"""
    import pyref
    return keyimg.strip(pyref.ntt_fast(pc, [v % pc.r for v in values], log_n, inverse=True))


def _oracle_image(pc, log_n, sel, sig, k, tabs, beta, compress, num_inputs, comms=None, is_merged=False):
    """The ProvingKey image of a circuit from oracle integers alone.  comms: (selector, sigma, plookup) points; None: [p(beta)] g."""
    import pyref
    n, gen = 1 << log_n, pyref.g1_gen(pc)
    sel_p, sig_p = [_coeffs(pc, log_n, s) for s in sel], [_coeffs(pc, log_n, s) for s in sig]
    tab_p = None if tabs is None else [_coeffs(pc, log_n, tabs[key]) for key in TABLES]
    commit = lambda p: pyref.g1_mul(pc, pyref.poly_eval(pc, p, beta), gen)
    if comms is None:
        comms = ([commit(p) for p in sel_p], [commit(p) for p in sig_p], None if tab_p is None else [commit(p) for p in tab_p])
    ck = [pyref.g1_mul(pc, pow(beta, i, pc.r), gen) for i in range(n + 3)]
    g2 = keyimg.g2_bytes(pc, compress)
    vk = dict(domain_size=n, num_inputs=num_inputs, sigma_comms=comms[1], selector_comms=comms[0], k=k, g=ck[0], h=bytes((7 * i + 1) % 256 for i in range(g2)),
              beta_h=bytes((5 * i + 2) % 256 for i in range(g2)), is_merged=is_merged, plookup_comms=comms[2])
    return keyimg.pk_image(pc, compress, sig_p, sel_p, ck, vk, tab_p), (sel_p, sig_p, tab_p)


def _prove(mj, c, prover, wires, pub, ultra):
    rng = mj.rng.test_rng()
    mj.rng.fr_rand(c, rng)                                         # (the draw of srs_beta comes first: snark.rs:495)
    blind = mj.snark.draw_blinders(c, rng, 6 if ultra else 5, ultra)
    return mj.snark.serialize_proof(c, prover.prove(wires, pub, mj.prover.TranscriptChallenges(prover, pub), blind))


def _old_way(mj, c, log_n, sel, sig, k, tabs, ck):
    """the prover of the same arrays through mzk_prover_create: coefficient forms by the product's own inverse NTT, uploaded from the host"""
    dom = mj.Radix2EvaluationDomain(c, log_n)
    kw = {"plookup": {name: dom.ifft(fr_mont_limbs(c, tabs[key])) for name, key in zip(mj.plonk.PLOOKUP_TABLE_POLYS, TABLES)}} if tabs is not None else {}
    return mj.prover.TurboPlonkProver(c, 1 << log_n, [dom.ifft(fr_mont_limbs(c, s)) for s in sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], k, ck, **kw)


def _vector(name, index):
    vecs = load_golden(name)
    return (vecs["proofs"] if name == "full_selector_proof_vectors" else vecs)[index]


@lru_cache(maxsize=None)
def _golden_case(name, index):
    """One committed vector: the circuit's integers rebuilt by the oracle's builder (as tests/test_golden_proofs_gpu.py::_general_case does)
    and its commitments as points."""
    import pyref
    import pyref_circuit as PC
    import pyref_verifier as V
    vec = _vector(name, index)
    pc, ultra = pyref.CURVES[vec["curve"]], vec["plonk_type"] == "UltraPlonk"
    rnd, gates, tabs = random.Random(vec["seed"]), vec.get("gates_mode", "hot"), None
    if ultra:
        sel, sig, k, w, pi, tabs = PC.general_ultra_circuit(pc, vec["log_n"], rnd, gates=gates)
    else:
        sel, sig, k, w, pi = PC.general_circuit(pc, vec["log_n"], rnd, gates=gates)
    assert ["%x" % x for x in pi[:4]] == vec["public_input"] and ["%x" % x for x in k] == vec["k"]
    pt = lambda h: V.g1_decompress(pc, bytes.fromhex(h))
    names = ("range_table_comm", "key_table_comm", "table_dom_sep_comm", "q_dom_sep_comm")
    comms = ([pt(h) for h in vec["selector_comms"]], [pt(h) for h in vec["sigma_comms"]], [pt(vec["plookup_comms"][x]) for x in names] if ultra else None)
    return vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms


GOLDEN = [pytest.param("general_proof_vectors", i, id=str(i)) for i in range(4)] + [pytest.param("full_selector_proof_vectors", i, id="all-%d" % i) for i in range(4)]


@pytest.mark.parametrize("name,index", GOLDEN)
def test_golden_keys_load_prove_and_save_byte_for_byte(gpu, mj, name, index):
    vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms = _golden_case(name, index)
    c, log_n, beta, pub = mj.params.CURVES[vec["curve"]], vec["log_n"], int(vec["srs_beta"], 16), pi[:4]
    wires = np.stack([fr_mont_limbs(c, col) for col in w])
    if name == "general_proof_vectors":
        assert None in comms[0], "q_ecc and friends are the zero polynomial here: infinity commitments"
    for compress in (True, False):
        im, _ = _oracle_image(pc, log_n, sel, sig, k, tabs, beta, compress, len(pub), comms)
        image = bytes(im.data)
        if compress:                                               # the records in the image are the vector's own
            at = im.layout["selector_comms_off"]
            assert image[at:at + len(comms[0]) * len(bytes.fromhex(vec["selector_comms"][0]))].hex() == "".join(vec["selector_comms"])
        key = mj.ProvingKey.deserialize(c, image, compress=compress, validate=True, check_commitments=True)
        assert (key.vk.domain_size, key.vk.num_inputs, key.vk.k, key.prover.ultra) == (1 << log_n, 4, list(k), ultra)
        assert _prove(mj, c, key.prover, wires, pub, ultra).hex() == vec["proof"]
        vk_slice = image[im.layout["vk_off"]:im.layout["vk_off"] + im.layout["vk_len"]]
        assert key.serialize() == image
        assert key.prover.serialize_vk(len(pub), key.vk.h, key.vk.beta_h, False, compress) == vk_slice == key.vk.serialize()
        # the same bytes from a prover built the old way (mzk_prover_create from host arrays), then saved
        old = _old_way(mj, c, log_n, sel, sig, k, tabs, key.commit_key)
        assert old.serialize_key(len(pub), key.vk.h, key.vk.beta_h, False, compress) == image
        assert old.serialize_vk(len(pub), key.vk.h, key.vk.beta_h, False, compress) == vk_slice
        old.release()
        key.release()


def _hand_circuit(pc, log_n, seed):
    """A TurboPlonk circuit for ANY domain size, with short polynomials: w_4 = w_0 + q_c on every row, no copy constraints (sigma is the
    identity), no public input.  q_lc[0] and q_o are the constant 1 (polynomials of length 1), q_c the values of a random polynomial of
    length n - 1, every other selector the zero polynomial (length 0)."""
    import pyref
    import pyref_circuit as PC
    n, r, rnd = 1 << log_n, pc.r, random.Random(seed)
    k = PC.general_circuit(pc, 4, random.Random(1))[2]
    q_c = pyref.ntt_fast(pc, [rnd.randrange(1, r) for _ in range(n - 1)] + [0], log_n)
    sel = [[0] * n for _ in range(13)]
    sel[0], sel[10], sel[11] = [1] * n, [1] * n, q_c
    w_n = pc.root_of_unity(log_n)
    sig = [[k[i] * pow(w_n, j, r) % r for j in range(n)] for i in range(5)]
    w = [[rnd.randrange(r) for _ in range(n)] for _ in range(4)]
    w.append([(w[0][j] + q_c[j]) % r for j in range(n)])
    return sel, sig, k, w


@pytest.mark.parametrize("curve_id,log_n", [(0, 3), (1, 2), (1, 5)])
def test_smallest_domains_and_short_polynomials(gpu, mj, curve_id, log_n):
    """n = 8, n = 4 (the tiny-domain quotient path, and k's five elements over rows of four) and a key whose polynomials have lengths 1,
    n - 1 and 0: the zero fill on load and the degree on save."""
    import pyref
    pc, c, beta = pyref.CURVES[curve_id], mj.params.CURVES[curve_id], 0x5EED5 + log_n
    sel, sig, k, w = _hand_circuit(pc, log_n, 77 + log_n)
    wires = np.stack([fr_mont_limbs(c, col) for col in w])
    im, (sel_p, _, _) = _oracle_image(pc, log_n, sel, sig, k, None, beta, True, 0)
    assert [len(p) for p in sel_p] == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, (1 << log_n) - 1, 0]
    image = bytes(im.data)
    key = mj.ProvingKey.deserialize(c, image, check_commitments=True, lagrange=(log_n == 5))
    old = _old_way(mj, c, log_n, sel, sig, k, None, key.commit_key)
    assert _prove(mj, c, key.prover, wires, [], False) == _prove(mj, c, old, wires, [], False)
    assert key.serialize() == image == old.serialize_key(0, key.vk.h, key.vk.beta_h)
    assert (key.lagrange_key is not None) == (log_n == 5)
    old.release()
    key.release()


def test_key_from_circuit_structure_saves_the_oracle_image(gpu, mj):
    """TurboPlonkProver.from_circuit (preprocess on the device), then saved: the bytes of the oracle-made image of the same circuit with
    the canonical sigma of its variable table (tests/test_preprocess_structure_gpu.py::_general)."""
    import pyref
    import pyref_circuit as PC
    pc, c, log_n, beta = pyref.CURVES[1], mj.params.CURVES[1], 4, 0xBEEF
    sel, sig, k, w, pi, tabs = PC.general_ultra_circuit(pc, log_n, random.Random(9100))
    var, n_vars = REF.wire_variables_from_sigma(pc, sig, k, log_n)
    n, W, r, w_n = 1 << log_n, 6, pc.r, pc.root_of_unity(log_n)
    cells = {}
    for i in range(W):
        for j in range(n):
            cells.setdefault(var[i][j], []).append((i, j))
    nxt = {cell: lst[(q + 1) % len(lst)] for lst in cells.values() for q, cell in enumerate(lst)}
    canon = [[k[nxt[(i, j)][0]] * pow(w_n, nxt[(i, j)][1], r) % r for j in range(n)] for i in range(W)]
    im, _ = _oracle_image(pc, log_n, sel, canon, k, tabs, beta, True, 4)
    limbs = lambda rows: np.stack([fr_mont_limbs(c, row) for row in rows])
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, n + 2)
    p = mj.prover.TurboPlonkProver.from_circuit(c, n, limbs(sel), np.array(var, dtype=np.uint32), n_vars, k, ck, table_values=limbs([tabs[key] for key in TABLES]))
    g2 = keyimg.g2_bytes(pc)
    assert p.serialize_key(4, bytes(im.data[im.layout["h_off"]:im.layout["h_off"] + g2]), bytes(im.data[im.layout["beta_h_off"]:im.layout["beta_h_off"] + g2])) == bytes(im.data)
    p.release()
    ck.release()


# ---- rejections --------------------------------------------------------------------------------------------------------------------------
def _ultra_vector():
    return next(("general_proof_vectors", i) for i in range(4) if _vector("general_proof_vectors", i)["plonk_type"] == "UltraPlonk" and _vector("general_proof_vectors", i)["curve"] == 0)


def _memory(gpu):
    import torch
    ws = C.c_uint64()
    assert gpu.load().mzk_workspace_hbm_bytes(C.byref(ws)) == 0
    torch.cuda.synchronize()
    return ws.value, torch.cuda.mem_get_info()[0]


def test_bad_keys_are_refused_naming_field_and_index_and_leave_nothing_behind(gpu, mj):
    import pyref
    vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms = _golden_case(*_ultra_vector())
    assert ultra and pc.curve_id == 0
    c, log_n, beta = mj.params.CURVES[0], vec["log_n"], int(vec["srs_beta"], 16)
    im, _ = _oracle_image(pc, log_n, sel, sig, k, tabs, beta, True, 4, comms)
    image, lay = bytes(im.data), im.layout
    mj.ProvingKey.deserialize(c, image, check_commitments=True).release()           # (the MSM scratch of the commitment check exists from here on)
    before = _memory(gpu)

    def refused(data, field, index, needle, **kw):
        with pytest.raises(mj.keys.KeySerializationError) as e:
            mj.ProvingKey.deserialize(c, bytes(data), **kw)
        assert (e.value.field, e.value.index) == (field, index) and needle in e.value.reason, e.value.reason
        assert isinstance(e.value, mj.SerializationError)
        assert _memory(gpu) == before, "a failed load leaves the workspace and the free memory as they were"

    r_rec = pc.r.to_bytes(32, "little")
    bad = bytearray(image)
    off, cnt = lay["sigmas"][2]
    assert cnt > 5
    bad[off + 32 * 5:off + 32 * 6] = r_rec
    refused(bad, "sigmas[2]", 5, "sigmas[2] coefficient 5: not below the modulus")
    bad = bytearray(image)
    off, cnt = lay["tables"][3]                                      # the last table polynomial: after the is_merged byte, an odd offset
    assert off % 2 == 1 and cnt > 0
    bad[off + 32 * (cnt - 1):off + 32 * cnt] = r_rec
    refused(bad, "plookup_pk.q_dom_sep_poly", cnt - 1, "not below the modulus")
    # a point on the curve but outside G1 as commit-key point 7 (validation on); accepted unchecked
    x = next(x for x in range(1, 100) if pow(x**3 + 4, (pc.q - 1) // 2, pc.q) == 1)
    y = pow(x**3 + 4, (pc.q + 1) // 4, pc.q)
    assert pyref.g1_on_curve(pc, (x, y)) and pyref.g1_mul(pc, pc.r, (x, y)) is not None
    bad = bytearray(image)
    bad[lay["commit_key_off"] + 48 * 7:lay["commit_key_off"] + 48 * 8] = keyimg.g1_record(pc, (x, y))
    refused(bad, "commit_key", 7, "commit_key point 7: not in the subgroup", validate=True)
    # one valid-but-changed coefficient: refused with check_commitments, loads without
    bad = bytearray(image)
    off, cnt = lay["selectors"][0]
    bad[off + 32:off + 64] = ((int.from_bytes(bad[off + 32:off + 64], "little") + 1) % pc.r).to_bytes(32, "little")
    refused(bad, "vk.selector_comms[0]", 0, "vk.selector_comms[0] does not commit selectors[0]", check_commitments=True)
    mj.ProvingKey.deserialize(c, bytes(bad)).release()
    bad = bytearray(image)
    off, cnt = lay["sigmas"][4]
    bad[off:off + 32] = (1).to_bytes(32, "little")
    refused(bad, "vk.sigma_comms[4]", 4, "does not commit sigmas[4]", check_commitments=True)
    # the container's own errors come through with their field
    refused(image[:-1], "plookup_pk.q_dom_sep_poly", None, "truncated in plookup_pk.q_dom_sep_poly")
    assert _memory(gpu) == before


def test_commit_key_passed_in_serves_two_keys_and_the_embedded_points_are_skipped(gpu, mj):
    vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms = _golden_case("full_selector_proof_vectors", 0)
    c, log_n, beta, pub = mj.params.CURVES[vec["curve"]], vec["log_n"], int(vec["srs_beta"], 16), pi[:4]
    wires = np.stack([fr_mont_limbs(c, col) for col in w])
    im, _ = _oracle_image(pc, log_n, sel, sig, k, tabs, beta, True, 4, comms)
    image = bytearray(im.data)
    at, cnt = im.layout["commit_key_off"], im.layout["commit_key_count"]
    rec = len(keyimg.g1_record(pc, None))
    image[at + rec:at + cnt * rec] = b"\xff" * ((cnt - 1) * rec)     # no point at all: reading them would fail (point 0 stays: vk.g is compared with the HANDLE's)
    with pytest.raises(mj.keys.KeySerializationError):
        mj.ProvingKey.deserialize(c, bytes(image))
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, beta, (1 << log_n) + 2)
    a = mj.ProvingKey.deserialize(c, bytes(image), commit_key=ck, check_commitments=True)
    b = mj.ProvingKey.deserialize(c, bytes(image), commit_key=ck)
    assert a.commit_key is ck and b.commit_key is ck and a._owned == [] and a.prover.handle != b.prover.handle
    assert _prove(mj, c, a.prover, wires, pub, ultra).hex() == vec["proof"] == _prove(mj, c, b.prover, wires, pub, ultra).hex()
    a.release()
    assert _prove(mj, c, b.prover, wires, pub, ultra).hex() == vec["proof"]
    b.release()
    ck.release()


def test_loaded_ultraplonk_key_recovers_its_variables_and_checks_a_witness(gpu, mj):
    vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms = _golden_case(*_ultra_vector())
    c, log_n, beta, pub = mj.params.CURVES[0], vec["log_n"], int(vec["srs_beta"], 16), pi[:4]
    wires = np.stack([fr_mont_limbs(c, col) for col in w])
    im, _ = _oracle_image(pc, log_n, sel, sig, k, tabs, beta, True, 4, comms)
    key = mj.ProvingKey.deserialize(c, bytes(im.data))
    var, n_vars = REF.wire_variables_from_sigma(pc, sig, k, log_n)
    assert key.prover.derive_wire_variables() == n_vars
    rep = key.prover.check_witness(wires, pub)
    assert rep.satisfied and rep.copy_checked
    n = 1 << log_n
    flat = [var[i][j] for i in range(6) for j in range(n)]
    cell = next(t for t in range(6 * n) if flat.index(flat[t]) < t)               # a cell that is not the representative of its variable
    wire, row_ = divmod(cell, n)
    bad = wires.copy()
    bad[wire, row_] = fr_mont_limbs(c, [(w[wire][row_] + 1) % pc.r])[0]
    rep = key.prover.check_witness(bad, pub)
    assert not rep.satisfied and rep.copy_checked and rep.copy_failures == 1 and rep.copy_cell == (wire, row_)
    key.release()


def test_cpp_host_saves_and_loads_the_same_image(gpu, mj, tmp_path):
    """`mzk_prove .. file C --save-pk F` then `.. file C --pk F --pk-check`: the same proof bytes (the golden vector's), F the image the
    Python side writes and the oracle-made one (this host writes zero bytes for the G2 elements, which it does not have)."""
    from importlib import import_module
    vec, pc, ultra, (sel, sig, k, w, pi, tabs), comms = _golden_case(*_ultra_vector())
    c, log_n, beta, pub = mj.params.CURVES[0], vec["log_n"], int(vec["srs_beta"], 16), pi[:4]
    circuit, saved = str(tmp_path / "circuit.bin"), str(tmp_path / "pk.bin")
    import_module("mpc-jellyfish_amd.circuit_io").write_circuit(circuit, c, log_n, sel, sig, k, w, pub_input=pub, tables=tabs)
    exe = os.path.join(ROOT, "mpc-jellyfish_amd", "mzk_prove")

    def run(*extra):
        out = subprocess.run([exe, "0", "file", circuit, "0", *extra], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
        return out.stdout.strip().splitlines(), json.loads(out.stdout.strip().splitlines()[-1])

    _, first = run("--save-pk", saved)
    lines, second = run("--pk", saved, "--pk-check", "--check-witness", "--derive-variables")
    assert first["proof_hex"] == second["proof_hex"] == vec["proof"] and first["vk_hex"] == second["vk_hex"]
    assert any(l.startswith("witness: satisfied") for l in lines)
    image = open(saved, "rb").read()
    assert first["pk_bytes"] == second["pk_bytes"] == len(image)
    im, _ = _oracle_image(pc, log_n, sel, sig, k, tabs, beta, True, 4, comms)
    want, g2 = bytearray(im.data), keyimg.g2_bytes(pc)
    want[im.layout["h_off"]:im.layout["h_off"] + 2 * g2] = bytes(2 * g2)
    assert image == bytes(want)
    key = mj.ProvingKey.deserialize(c, image, check_commitments=True)
    assert key.serialize() == image
    key.release()
    # a changed coefficient is refused by --pk-check, naming the field
    bad = bytearray(image)
    off, _ = im.layout["selectors"][0]
    bad[off] ^= 1
    open(saved, "wb").write(bytes(bad))
    out = subprocess.run([exe, "0", "file", circuit, "0", "--pk", saved, "--pk-check"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "vk.selector_comms[0] does not commit selectors[0]" in out.stdout + out.stderr


def test_reference_proving_keys_when_present(gpu, mj):
    path = os.path.join(ROOT, "tests", "golden", "ref_proving_keys.json")
    if not os.path.exists(path):
        pytest.skip("parity unpinned: tests/golden/ref_proving_keys.json (integration/rust gen_fixtures, family proving_key) has not been generated")
    for case in json.load(open(path)):
        c = mj.params.CURVES[case["curve"]]
        for mode, compress in (("pk_compressed", True), ("pk_uncompressed", False)):
            image = bytes.fromhex(case[mode])
            key = mj.ProvingKey.deserialize(c, image, compress=compress, check_commitments=True)
            assert key.serialize() == image
            if compress:
                assert key.prover.serialize_vk(key.vk.num_inputs, key.vk.h, key.vk.beta_h, key.vk.is_merged) == bytes.fromhex(case["vk_compressed"])
            key.release()
