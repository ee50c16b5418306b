"""CPU suite: mzk_batch_proof_layout (include/mzk.h; host-only, no GPU and no mzk_init) against oracle/pyref_verifier.deserialize_batch_proof on the
golden BatchProofs: the image length, every offset the layout names, and the container check that mzk_verifier_aggregate_begin runs on the host
before anything is staged (length, every Vec count, every Option tag)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import pyref_fs as FS

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_ENCODING = -1, -5, -11


def _golden_batch_proofs():
    """(curve id, ultra, image) of every `batch_proof` in the two golden files"""
    out = []

    def walk(x):
        if isinstance(x, dict):
            if "batch_proof" in x:
                out.append((x["curve"], x["plonk_type"] == "UltraPlonk", bytes.fromhex(x["batch_proof"])))
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)
    walk(load_golden("batch_vectors"))
    n = len(out)
    walk(load_golden("full_selector_proof_vectors"))
    assert n >= 1 and len(out) > n
    return out


GOLDEN = _golden_batch_proofs()


def _layout(mj, cid, ultra, m, image=None, compress=True):
    return mj.keys.batch_proof_layout(cid, ultra, m, compress, image)


@pytest.mark.parametrize("n", range(len(GOLDEN)))
def test_layout_is_the_oracles_parse(mj, pyref, n):
    import pyref_verifier as V
    cid, ultra, blob = GOLDEN[n]
    pc = pyref.CURVES[cid]
    bp = V.deserialize_batch_proof(pc, blob)
    m, W = len(bp["prod_perm_poly_comms_vec"]), 6 if ultra else 5
    G = 48 if cid == 0 else 32
    L = _layout(mj, cid, ultra, m, blob)                              # (with the image: its container is accepted)
    assert (L.m, L.num_wire_types, L.ultra, L.g1_record_bytes, L.total_len) == (m, W, int(ultra), G, len(blob))
    g1 = lambda off, pt: blob[off:off + G] == FS.g1_bytes(pc, pt)
    fr = lambda off, v: blob[off:off + 32] == v.to_bytes(32, "little")
    for j in range(m):
        ev, pl = bp["poly_evals_vec"][j], bp["plookup_proofs_vec"][j]
        assert all(g1(L.wires_off[j] + k * G, pt) for k, pt in enumerate(bp["wires_poly_comms_vec"][j])) and len(bp["wires_poly_comms_vec"][j]) == W
        assert g1(L.prod_perm_off[j], bp["prod_perm_poly_comms_vec"][j])
        assert all(fr(L.wires_evals_off[j] + 32 * k, v) for k, v in enumerate(ev["wires_evals"])) and len(ev["wires_evals"]) == W
        assert all(fr(L.sigma_evals_off[j] + 32 * k, v) for k, v in enumerate(ev["wire_sigma_evals"])) and len(ev["wire_sigma_evals"]) == W - 1
        assert fr(L.perm_next_off[j], ev["perm_next_eval"])
        assert blob[L.plookup_tag_off[j]] == int(ultra) and (pl is not None) == ultra
        if ultra:
            assert g1(L.h_off[j], pl["h_poly_comms"][0]) and g1(L.h_off[j] + G, pl["h_poly_comms"][1]) and g1(L.prod_lookup_off[j], pl["prod_lookup_poly_comm"])
            assert all(fr(L.plookup_evals_off[j] + 32 * k, pl["evals"][name]) for k, name in enumerate(V.PLOOKUP_EVAL_FIELDS))
        else:
            assert (L.h_off[j], L.prod_lookup_off[j], L.plookup_evals_off[j]) == (0, 0, 0)
    assert all(g1(L.split_quot_off + k * G, pt) for k, pt in enumerate(bp["split_quot_poly_comms"])) and len(bp["split_quot_poly_comms"]) == W
    assert g1(L.opening_off, bp["opening_proof"]) and g1(L.shifted_opening_off, bp["shifted_opening_proof"])
    assert L.shifted_opening_off + G == len(blob)


@pytest.mark.parametrize("cid,ultra,compress", [(0, False, True), (1, True, True), (0, True, False), (1, False, False)])
def test_lengths_follow_the_format(mj, cid, ultra, compress):
    """the length from the format as include/mzk.h states it, for m = 1, 2, 64 in both modes; m = 1 is a Proof's records regrouped"""
    G, W = (48 if cid == 0 else 32) * (1 if compress else 2), 6 if ultra else 5
    for m in (1, 2, 64):
        want = 8 + m * (8 + W * G) + 8 + m * G + 8 + m * (8 + 32 * W + 8 + 32 * (W - 1) + 32) + 8 + m * (1 + (8 + 3 * G + 32 * 15 if ultra else 0)) + 8 + W * G + 2 * G
        assert _layout(mj, cid, ultra, m, compress=compress).total_len == want


def test_instance_counts_out_of_range_are_refused(mj):
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")
    L = mj.load()
    out = lib.BatchProofLayout()
    assert lib.MAX_INSTANCES == 64
    assert L.mzk_batch_proof_layout(0, 0, 0, 1, None, 0, C.byref(out)) == ERR_INVALID_ARG
    assert L.mzk_batch_proof_layout(0, 0, 65, 1, None, 0, C.byref(out)) == ERR_UNSUPPORTED and b"64" in L.mzk_last_error()
    assert L.mzk_batch_proof_layout(0, 0, 64, 1, None, 0, C.byref(out)) == 0 and out.m == 64
    assert L.mzk_batch_proof_layout(0, 2, 1, 1, None, 0, C.byref(out)) == ERR_INVALID_ARG
    assert L.mzk_batch_proof_layout(7, 0, 1, 1, None, 0, C.byref(out)) == ERR_INVALID_ARG
    assert L.mzk_batch_proof_layout(0, 0, 1, 1, None, 0, None) == ERR_INVALID_ARG


@pytest.mark.parametrize("n", range(len(GOLDEN)))
def test_container_defects_are_refused_on_the_host(mj, pyref, n):
    cid, ultra, blob = GOLDEN[n]
    m = int.from_bytes(blob[:8], "little")
    W = 6 if ultra else 5
    L = _layout(mj, cid, ultra, m)
    E = mj.keys.ProofEncodingError

    def refused(image, instance, field, reason):
        with pytest.raises(E) as e:
            _layout(mj, cid, ultra, m, image)
        assert (e.value.instance, e.value.field) == (instance, field) and reason in e.value.reason, e.value.reason
        assert e.value.reason.startswith(f"instance {instance}: {field}: ")

    def with_count(off, value):
        bad = bytearray(blob)
        bad[off:off + 8] = value.to_bytes(8, "little")
        return bytes(bad)
    refused(blob[:-1], m, "length", f"{len(blob) - 1} bytes, expected {len(blob)}")
    refused(blob + b"\0", m, "length", f"{len(blob) + 1} bytes, expected {len(blob)}")
    refused(with_count(0, m + 1), m, "wires_poly_comms_vec.len", f"{m + 1}, expected {m}")
    last = m - 1
    refused(with_count(L.wires_off[last] - 8, W - 1), last, "wires_poly_comms.len", f"{W - 1}, expected {W}")
    refused(with_count(L.prod_perm_off[0] - 8, 0), m, "prod_perm_poly_comms_vec.len", f"0, expected {m}")
    refused(with_count(L.wires_evals_off[0] - 16, 2**64 - 1), m, "poly_evals_vec.len", f"{2**64 - 1}, expected {m}")
    refused(with_count(L.wires_evals_off[last] - 8, W + 1), last, "wires_evals.len", f"{W + 1}, expected {W}")
    refused(with_count(L.sigma_evals_off[0] - 8, W), 0, "wire_sigma_evals.len", f"{W}, expected {W - 1}")
    refused(with_count(L.plookup_tag_off[0] - 8, m - 1), m, "plookup_proofs_vec.len", f"{m - 1}, expected {m}")
    refused(with_count(L.split_quot_off - 8, W - 1), m, "split_quot_poly_comms.len", f"{W - 1}, expected {W}")
    tag = bytearray(blob)
    tag[L.plookup_tag_off[last]] ^= 1
    refused(bytes(tag), last, "plookup_proof", "key")
    tag[L.plookup_tag_off[last]] = 2
    refused(bytes(tag), last, "plookup_proof", "invalid Option tag")
    if ultra:
        refused(with_count(L.h_off[0] - 8, 3), 0, "plookup_proof.h_poly_comms.len", "3, expected 2")
    # two defects: the first in image order is the one reported
    both = bytearray(with_count(L.split_quot_off - 8, W + 1))
    both[L.plookup_tag_off[0]] = 3
    refused(bytes(both), 0, "plookup_proof", "invalid Option tag")
    # the other type's layout does not fit this image
    with pytest.raises(E):
        _layout(mj, cid, not ultra, m, blob)
