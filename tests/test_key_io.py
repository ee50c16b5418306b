"""CPU: the host-only container parser of a serialized ProvingKey / VerifyingKey (csrc/keyfmt.hpp behind mzk_key_layout; format in
include/mzk.h).  Images are built here from oracle/pyref_fs.fr_bytes / g1_bytes / vec_bytes and the format (tests/keyimg.py), for both
curves, both modes, TurboPlonk and UltraPlonk at n = 8: the parser must report the offsets and counts the builder recorded, refuse every
proper prefix naming the field the cut falls in, refuse each structural defect of the list in the header, and survive -- as a stand-alone
program under AddressSanitizer and UBSan (tools/key_layout_check.cpp), never as code loaded into Python -- every truncation and every
small / 0xFF value in every byte of every length prefix and tag."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import keyimg
import pyref
import pyref_fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
ERR_ENCODING = -11
CASES = [(cid, compress, ultra) for cid in (0, 1) for compress in (True, False) for ultra in (False, True)]


def _image(cid, compress, ultra, n=N, mutate=None):
    """A well-formed image with polynomials of every kind of length: full, short, one coefficient, zero."""
    pc = pyref.CURVES[cid]
    W, nsel = (6, 14) if ultra else (5, 13)
    gen = pyref.g1_gen(pc)
    pts = [pyref.g1_mul(pc, i + 1, gen) for i in range(n + 3)]
    lens = [n, n - 1, 1, 0, n, 3, n, n, 2, n, 0, n, n, 1]
    poly = lambda seed, ln: [(seed * 1000003 + 7 * j + 1) % pc.r for j in range(ln)]
    spec = dict(
        sigmas=[poly(100 + i, n) for i in range(W)],
        selectors=[poly(200 + i, lens[i]) for i in range(nsel)],
        commit_key=pts,
        vk=dict(domain_size=n, num_inputs=3, sigma_comms=pts[:W], selector_comms=[None if lens[i] == 0 else pts[i % len(pts)] for i in range(nsel)],
                k=[(i + 1) * 7 for i in range(W)], g=pts[0], h=bytes(range(1, 1 + keyimg.g2_bytes(pc, compress))),
                beta_h=bytes(range(2, 2 + keyimg.g2_bytes(pc, compress))), is_merged=ultra, plookup_comms=pts[1:5] if ultra else None),
        tables=[poly(300, n), poly(301, 0), poly(302, n - 1), poly(303, 1)] if ultra else None)
    if mutate:
        mutate(spec)
    return pc, keyimg.pk_image(pc, compress, **spec)


def _layout(mj, cid, data, compress=True, vk_only=False):
    """(rc, KeyLayout, message)"""
    L = mj.load()
    lib = __import__("importlib").import_module("mpc-jellyfish_amd.lib")
    out = lib.KeyLayout()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    rc = L.mzk_key_layout(cid, buf, len(data), (1 if compress else 0) | (8 if vk_only else 0), C.byref(out))
    return rc, out, L.mzk_last_error().decode() if rc else ""


def _refused(mj, cid, data, *needles, compress=True):
    rc, _, msg = _layout(mj, cid, data, compress)
    assert rc == ERR_ENCODING, (rc, msg)
    for s in needles:
        assert s in msg, msg
    return msg


@pytest.mark.parametrize("cid,compress,ultra", CASES)
def test_layout_reports_the_offsets_and_counts_of_the_builder(mj, cid, compress, ultra):
    pc, im = _image(cid, compress, ultra)
    rc, lay, msg = _layout(mj, cid, im.data, compress)
    assert rc == 0, msg
    want, W, nsel = im.layout, 6 if ultra else 5, 14 if ultra else 13
    assert (lay.num_wire_types, lay.num_selectors, lay.has_plookup, lay.has_plookup_vk, lay.is_merged) == (W, nsel, int(ultra), int(ultra), int(ultra))
    assert (lay.domain_size, lay.num_inputs, lay.total_len) == (N, 3, len(im.data))
    assert lay.g1_record_bytes == len(keyimg.g1_record(pc, None, compress)) and lay.g2_record_bytes == keyimg.g2_bytes(pc, compress)
    assert [(lay.sigma_off[i], lay.sigma_len[i]) for i in range(W)] == want["sigmas"]
    assert [(lay.selector_off[i], lay.selector_len[i]) for i in range(nsel)] == want["selectors"]
    assert [(lay.table_off[i], lay.table_len[i]) for i in range(4 if ultra else 0)] == want["tables"]
    assert (lay.commit_key_off, lay.commit_key_count) == (want["commit_key_off"], N + 3)
    assert (lay.vk_off, lay.vk_len) == (want["vk_off"], want["vk_len"])
    for key in ("sigma_comms_off", "selector_comms_off", "k_off", "g_off", "h_off", "beta_h_off") + (("plookup_comms_off",) if ultra else ()):
        assert getattr(lay, key) == want[key], key
    # the embedded VerifyingKey alone parses the same way, with offsets relative to its own start
    vk = bytes(im.data[lay.vk_off:lay.vk_off + lay.vk_len])
    rc, v, msg = _layout(mj, cid, vk, compress, vk_only=True)
    assert rc == 0, msg
    assert (v.num_wire_types, v.num_selectors, v.domain_size, v.num_inputs, v.vk_off, v.vk_len, v.total_len) == (W, nsel, N, 3, 0, len(vk), len(vk))
    assert (v.k_off, v.g_off, v.beta_h_off) == tuple(want[k] - want["vk_off"] for k in ("k_off", "g_off", "beta_h_off"))
    assert _layout(mj, cid, vk[:-1], compress, vk_only=True)[0] == ERR_ENCODING


@pytest.mark.parametrize("cid,compress,ultra", [(0, True, True), (1, False, False)])
def test_every_proper_prefix_is_refused_naming_the_field_of_the_cut(mj, cid, compress, ultra):
    _, im = _image(cid, compress, ultra)
    for cut in range(len(im.data)):
        _refused(mj, cid, im.data[:cut], f"truncated in {im.field_at(cut)} at byte {cut}", compress=compress)


def _set_u64(im, name, value, nth=0):
    off = [a for n_, a, _ in im.spans if n_ == name][nth]
    im.data[off:off + 8] = struct.pack("<Q", value)


def _set_byte(im, name, value):
    off = next(a for n_, a, _ in im.spans if n_ == name)
    im.data[off] = value


def test_each_structural_rejection(mj):
    n = N
    turbo = lambda m=None: _image(0, True, False, mutate=m)[1]
    ultra = lambda m=None: _image(1, True, True, mutate=m)[1]
    # a bool / an Option tag that is neither 0 nor 1
    for name in ("vk.is_merged", "vk.plookup_vk", "plookup_pk"):
        im = turbo()
        _set_byte(im, name, 2)
        _refused(mj, 0, im.data, name, "neither 0 nor 1")
    # a sigma count that is not 5 or 6; a selector count that does not go with W
    _refused(mj, 0, turbo(lambda s: s["sigmas"].pop()).data, "sigmas: count 4")
    _refused(mj, 0, turbo(lambda s: s["sigmas"].extend([[1]] * 2)).data, "sigmas: count 7")
    _refused(mj, 0, turbo(lambda s: s["selectors"].append([1])).data, "selectors: count 14 is not 13")
    _refused(mj, 1, ultra(lambda s: s["selectors"].pop()).data, "selectors: count 13 is not 14")
    # plookup_pk and plookup_vk not both present or both absent; then, both alike, present when W is not 6 / absent when it is
    both = "plookup_pk and vk.plookup_vk are not both present or both absent"
    _refused(mj, 0, turbo(lambda s: s.update(tables=[[1]] * 4)).data, both)
    _refused(mj, 1, ultra(lambda s: s.update(tables=None)).data, both)
    _refused(mj, 1, ultra(lambda s: s["vk"].update(plookup_comms=None)).data, both)
    _refused(mj, 0, turbo(lambda s: (s.update(tables=[[1]] * 4), s["vk"].update(plookup_comms=[None] * 4))).data, "plookup_pk: present with 5 wire types")
    _refused(mj, 1, ultra(lambda s: (s.update(tables=None), s["vk"].update(plookup_comms=None))).data, "plookup_pk: absent with 6 wire types")
    vk_of = lambda im: bytes(im.data[im.layout["vk_off"]:im.layout["vk_off"] + im.layout["vk_len"]])
    rc, _, msg = _layout(mj, 0, vk_of(turbo(lambda s: (s.update(tables=[[1]] * 4), s["vk"].update(plookup_comms=[None] * 4)))), vk_only=True)
    assert rc == ERR_ENCODING and "vk.plookup_vk: present with 5 wire types" in msg, msg
    # counts inside vk that do not match W and nsel
    _refused(mj, 0, turbo(lambda s: s["vk"]["sigma_comms"].pop()).data, "vk.sigma_comms: count 4")
    _refused(mj, 0, turbo(lambda s: s["vk"]["selector_comms"].append(None)).data, "vk.selector_comms: count 14")
    _refused(mj, 0, turbo(lambda s: s["vk"]["k"].append(1)).data, "vk.k: count 6")
    # the domain size
    _refused(mj, 0, turbo(lambda s: s["vk"].update(domain_size=12)).data, "vk.domain_size", "not a power of two")
    _refused(mj, 0, turbo(lambda s: s["vk"].update(domain_size=0)).data, "vk.domain_size", "not a power of two")
    _refused(mj, 0, turbo(lambda s: s["vk"].update(domain_size=1 << 28)).data, "vk.domain_size", "above 2^27")
    # a polynomial longer than the domain; a commit key shorter than n + 3
    _refused(mj, 0, turbo(lambda s: s["selectors"][4].append(5)).data, "selectors[4]: 9 coefficients, more than the domain size 8")
    _refused(mj, 0, turbo(lambda s: s["sigmas"][1].append(5)).data, "sigmas[1]: 9 coefficients")
    _refused(mj, 1, ultra(lambda s: s["tables"][2].extend([5, 5])).data, "plookup_pk.table_dom_sep_poly: 9 coefficients")
    _refused(mj, 0, turbo(lambda s: s["commit_key"].pop()).data, f"commit_key: {n + 2} points, fewer than the domain size + 3")
    # bytes left over
    _refused(mj, 0, bytes(turbo().data) + b"\0", "1 bytes left over after the last field")
    # a polynomial with trailing zero coefficients is accepted, as ark accepts it; so is the zero polynomial (count 0: in every image here)
    assert _layout(mj, 0, turbo(lambda s: s["selectors"].__setitem__(5, [1, 0, 0])).data)[0] == 0


def test_counts_whose_product_would_overflow_are_truncated_not_wrapped(mj):
    for name, nth in (("sigmas[2].len", 0), ("selectors[0].len", 0), ("commit_key.len", 0), ("vk.sigma_comms.len", 0), ("vk.k.len", 0)):
        for value in (2**64 - 1, 2**59 + 1, 2**63):                # 32 (2^59 + 1) = 32 mod 2^64: a wrapped product would look small
            im = _image(0, True, False)[1]
            _set_u64(im, name, value, nth)
            msg = _refused(mj, 0, im.data)
            if name.startswith("vk."):                             # (a count inside vk is compared with W first)
                assert "count" in msg, msg
            else:
                assert msg == f"truncated in {name[:-4]} at byte {len(im.data)}", msg
    im = _image(0, True, False)[1]
    _set_u64(im, "sigmas.len", 2**64 - 1)
    _refused(mj, 0, im.data, "sigmas: count 18446744073709551615")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("key_layout_check") / "key_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "mpc-jellyfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "key_layout_check.cpp")])
    return exe


@pytest.mark.parametrize("cid,compress,ultra,vk_only", [(0, True, True, False), (1, False, False, False), (1, True, True, True)])
def test_parser_alone_under_sanitizers(checker, tmp_path, mj, cid, compress, ultra, vk_only):
    _, im = _image(cid, compress, ultra)
    data = bytes(im.data)
    if vk_only:
        data = data[im.layout["vk_off"]:im.layout["vk_off"] + im.layout["vk_len"]]
    path = tmp_path / "image.bin"
    path.write_bytes(data)
    out = subprocess.run([checker, str(path), str(cid), str((1 if compress else 0) | (8 if vk_only else 0))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok") and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, \
        out.stdout + out.stderr
    assert f"{len(data)} truncations refused" in out.stdout, out.stdout


def test_new_symbols_are_exported_and_declared(mj):
    L = mj.load()
    header = open(os.path.join(ROOT, "include", "mzk.h")).read()
    for name in ("mzk_key_layout", "mzk_fr_decode_dev", "mzk_fr_encode_dev", "mzk_prover_create_serialized", "mzk_prover_serialize_key", "mzk_prover_serialize_vk"):
        assert hasattr(L, name), name
        assert f"MZK_API int32_t {name}(" in header, name
    for text in ("MZK_KEY_CHECK_COMMITMENTS", "MZK_KEY_VK_ONLY", "mzk_key_layout_t"):
        assert text in header
    assert mj.ProvingKey and mj.VerifyingKey and mj.keys.KeySerializationError


def test_verifying_key_object_round_trips_a_bare_image(mj):
    for cid, compress, ultra in ((0, True, False), (1, False, True)):
        pc, im = _image(cid, compress, ultra)
        vk_bytes = bytes(im.data[im.layout["vk_off"]:im.layout["vk_off"] + im.layout["vk_len"]])
        vk = mj.VerifyingKey.deserialize(cid, vk_bytes, compress=compress)
        assert (vk.domain_size, vk.num_inputs, vk.is_merged, vk.k) == (N, 3, ultra, [(i + 1) * 7 for i in range(6 if ultra else 5)])
        assert len(vk.selector_comms) == (14 if ultra else 13) and (vk.plookup_comms is not None) == ultra
        assert vk.g == keyimg.g1_record(pc, pyref.g1_gen(pc), compress) and vk.serialize() == vk_bytes
        with pytest.raises(mj.keys.KeySerializationError) as e:
            mj.VerifyingKey.deserialize(cid, vk_bytes[:40], compress=compress)
        assert e.value.field == "vk.sigma_comms" and e.value.index is None
