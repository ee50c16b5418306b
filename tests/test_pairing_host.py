"""CPU: the host pairing (csrc/hostpairing.hpp behind mzk_g2_decode / mzk_g2_mul / mzk_pairing_product_is_one / mzk_pairing_gt) and the batch
challenge (csrc/merlin.cuh behind mzk_batch_verify_challenge), both curves, against oracle/pyref_pairing.py (pairings by the definition)
and oracle/pyref_fs.py.  No GPU and no mzk_init: the entry points are host-only.  G2 records are encoded HERE from the format in
include/mzk.h.  The towers, the final exponentiation and bilinearity also run as a stand-alone program under AddressSanitizer and UBSan
(tools/host_pairing_check.cpp), never as code loaded into Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref
import pyref_fs
import pyref_pairing as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ENCODING = -11
COMPRESSED, VALIDATE = 1, 2
A, B = 0x1234567, 0x89abcde


def _limbs(v, n):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)]


def _fq_mont(c, vals):
    """canonical ints -> one flat uint64 array of Montgomery Fq elements"""
    R = 1 << (64 * c.fq_limbs)
    return np.array([l for v in vals for l in _limbs(v % c.q * R % c.q, c.fq_limbs)], dtype=np.uint64)


def _g1(c, pts):
    return _fq_mont(c, [v for p in pts for v in ((0, 0) if p is None else p)])


def _g2(c, pts):
    return _fq_mont(c, [v for p in pts for v in (p[0].c[0], p[0].c[1], p[1].c[0], p[1].c[1])])


def g2_record(pc, pt, compressed, infinity=False):
    """ark-serialize 0.4, as include/mzk.h states it"""
    c, q = pc.c, pc.c.q
    (x0, x1), (y0, y1) = ((0, 0), (0, 0)) if infinity else (pt[0].c, pt[1].c)
    larger = not infinity and (y1, y0) > ((-y1) % q, (-y0) % q)
    if c.curve_id == 0:
        body = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big") + (b"" if compressed else y1.to_bytes(48, "big") + y0.to_bytes(48, "big")))
        body[0] |= (0x80 if compressed else 0) | (0x40 if infinity else 0) | (0x20 if compressed and larger else 0)
    else:
        body = bytearray(x0.to_bytes(32, "little") + x1.to_bytes(32, "little") + (b"" if compressed else y0.to_bytes(32, "little") + y1.to_bytes(32, "little")))
        body[-1] |= (0x40 if infinity else 0) | (0x80 if larger else 0)
    return bytes(body)


def _buf(data):
    return (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))


def _decode(L, cid, rec, flags):
    """(rc, point as pyref_pairing Fq2 pair or None, message)"""
    pc = PR.PAIRINGS[cid]
    c = pc.c
    out = np.zeros(4 * c.fq_limbs, dtype=np.uint64)
    rc = L.mzk_g2_decode(cid, _buf(rec), flags, out.ctypes.data)
    if rc:
        return rc, None, L.mzk_last_error().decode()
    rinv = pow(1 << (64 * c.fq_limbs), -1, c.q)
    v = [sum(int(out[i * c.fq_limbs + j]) << (64 * j) for j in range(c.fq_limbs)) * rinv % c.q for i in range(4)]
    return 0, (pc.Fq2(v[0:2]), pc.Fq2(v[2:4])), ""


def _gt(L, cid, p1, q2):
    pc = PR.PAIRINGS[cid]
    c = pc.c
    out = np.zeros(12 * c.fq_limbs, dtype=np.uint64)
    g1, g2 = _g1(c, [p1]), _g2(c, [q2])
    assert L.mzk_pairing_gt(cid, g1.ctypes.data, g2.ctypes.data, out.ctypes.data) == 0
    return pc.Fq12([sum(int(out[i * c.fq_limbs + j]) << (64 * j) for j in range(c.fq_limbs)) for i in range(12)])


def _is_one(L, cid, pairs):
    c = PR.PAIRINGS[cid].c
    g1, g2 = _g1(c, [p for p, _ in pairs]), _g2(c, [q for _, q in pairs])
    out = C.c_int32(-1)
    assert L.mzk_pairing_product_is_one(cid, g1.ctypes.data if pairs else None, g2.ctypes.data if pairs else None, len(pairs), C.byref(out)) == 0
    assert out.value in (0, 1)
    return bool(out.value)


def _fq2_sqrt(pc, a):
    """a square root in Fq2 (q = 3 mod 4), or None"""
    q, F = pc.c.q, pc.Fq2
    if a.is_zero():
        return a
    a1 = a ** ((q - 3) // 4)
    alpha = a1 * a1 * a
    x0 = a1 * a
    x = F([0, 1]) * x0 if alpha == F([-1]) else (F([1]) + alpha) ** ((q - 1) // 2) * x0
    return x if x * x == a else None


@pytest.fixture(scope="module")
def L(mj):
    return mj.load()


@pytest.fixture(scope="module")
def gen_pairing(L):
    """per curve: the library's e(G1, G2) on the generators and the oracle's"""
    out = {}
    for cid in (0, 1):
        pc = PR.PAIRINGS[cid]
        G = pyref.g1_gen(pc.c)
        out[cid] = (_gt(L, cid, G, pc.g2), pc.pairing(pc.g2, G))
    return out


@pytest.mark.parametrize("cid", [0, 1])
def test_gt_on_the_generators_is_the_oracles_pairing(cid, gen_pairing):
    pc = PR.PAIRINGS[cid]
    got, want = gen_pairing[cid]
    one = pc.Fq12.one()
    # include/mzk.h: BN254 the oracle's value, BLS12-381 its inverse (the Miller value is conjugated for the negative x)
    assert got == (want if cid == 1 else want.inv())
    assert got != one and got ** pc.c.r == one


@pytest.mark.parametrize("cid", [0, 1])
def test_gt_is_bilinear(cid, L, gen_pairing):
    pc = PR.PAIRINGS[cid]
    c = pc.c
    e = gen_pairing[cid][0]
    assert _gt(L, cid, pyref.g1_mul(c, A, pyref.g1_gen(c)), pc.g2_mul(pc.g2, B)) == e ** (A * B)
    assert _gt(L, cid, None, pc.g2) == pc.Fq12.one()                                  # (0, 0) is infinity


@pytest.mark.parametrize("cid", [0, 1])
def test_pairing_product_agrees_with_the_oracle(cid, L):
    pc = PR.PAIRINGS[cid]
    c = pc.c
    G = pyref.g1_gen(c)
    aG, nG = pyref.g1_mul(c, A, G), pyref.g1_neg(c, G)
    aQ, bQ = pc.g2_mul(pc.g2, A), pc.g2_mul(pc.g2, B)
    sets = [
        ([], True),
        ([(None, pc.g2)], True),
        ([(G, pc.g2)], False),
        ([(aG, pc.g2), (nG, aQ)], True),                                                # e(aG, Q) e(-G, aQ) = 1
        ([(aG, pc.g2), (nG, bQ)], False),
        ([(aG, pc.g2), (None, bQ), (nG, aQ)], True),
        ([(aG, pc.g2), (G, bQ), (nG, aQ)], False),
    ]
    assert sorted({len(s) for s, _ in sets}) == [0, 1, 2, 3]
    for pairs, want in sets:
        assert pc.multi_pairing_is_one(pairs) == want
        assert _is_one(L, cid, pairs) == want, pairs


@pytest.mark.parametrize("cid", [0, 1])
def test_g2_records_round_trip_and_g2_mul(cid, L):
    pc = PR.PAIRINGS[cid]
    c = pc.c
    beta = 0x1F2E3D4C5B6A79880123456789ABCDEF % c.r
    want = pc.g2_mul(pc.g2, beta)
    k = (C.c_uint64 * 4)(*_limbs(beta, 4))
    for compressed in (True, False):
        flags = COMPRESSED if compressed else 0
        n = (96 if cid == 0 else 64) * (1 if compressed else 2)
        for pt in (pc.g2, want, PR.ec_neg(want)):                                       # y and -y: both values of the sign flag
            rec = g2_record(pc, pt, compressed)
            assert len(rec) == n
            rc, got, msg = _decode(L, cid, rec, flags | VALIDATE)
            assert rc == 0 and got == pt, msg
            assert _decode(L, cid, rec, flags)[1] == pt
        out = (C.c_uint8 * n)()
        assert L.mzk_g2_mul(cid, None, k, flags, out) == 0                              # NULL: the standard generator
        assert bytes(out) == g2_record(pc, want, compressed)
        out2 = (C.c_uint8 * n)()
        k2 = (C.c_uint64 * 4)(*_limbs(B, 4))
        assert L.mzk_g2_mul(cid, _buf(bytes(out)), k2, flags | VALIDATE, out2) == 0     # [B]([beta]h) from its record
        assert bytes(out2) == g2_record(pc, pc.g2_mul(want, B), compressed)
        kr = (C.c_uint64 * 4)(*_limbs(c.r, 4))
        assert L.mzk_g2_mul(cid, None, kr, flags, out2) == 0 and bytes(out2) == g2_record(pc, None, compressed, infinity=True)


@pytest.mark.parametrize("cid", [0, 1])
def test_g2_decode_refuses(cid, L):
    pc = PR.PAIRINGS[cid]
    c, q = pc.c, pc.c.q
    F = pc.Fq2

    def refused(rec, flags, reason):
        rc, _, msg = _decode(L, cid, rec, flags)
        assert rc == ERR_ENCODING and msg == "G2: " + reason, (rc, msg)

    good_c, good_u = g2_record(pc, pc.g2, True), g2_record(pc, pc.g2, False)
    # flags
    if cid == 0:
        refused(bytes([good_c[0] & 0x7F]) + good_c[1:], COMPRESSED, "invalid flag bits")              # compressed bit missing
        refused(bytes([good_u[0] | 0x80]) + good_u[1:], 0, "invalid flag bits")
        refused(bytes([good_u[0] | 0x20]) + good_u[1:], 0, "invalid flag bits")
    else:
        refused(good_c[:-1] + bytes([good_c[-1] | 0xC0]), COMPRESSED, "invalid flag bits")
        refused(good_u[:-1] + bytes([good_u[-1] | 0xC0]), 0, "invalid flag bits")
    # infinity is refused
    refused(g2_record(pc, None, True, infinity=True), COMPRESSED, "point at infinity")
    refused(g2_record(pc, None, False, infinity=True), 0, "point at infinity")
    # x >= q in either coordinate half; y >= q uncompressed
    for x in ((q, 0), (0, q), (q + 5, 1)):
        refused(_raw(pc, x, (0, 0), True), COMPRESSED, "coordinate not below the field modulus")
    refused(_raw(pc, pc.g2[0].c, (1, q), False), 0, "coordinate not below the field modulus")
    # a non-square x^3 + b', and a point of the twist outside G2
    non_square = off_subgroup = None
    for k in range(1, 200):
        x = F([k, 1])
        y = _fq2_sqrt(pc, x * x * x + pc.b2)
        if y is None:
            non_square = non_square or x
        elif off_subgroup is None and PR.ec_mul((x, y), c.r) is not None:
            off_subgroup = (x, y)
        if non_square is not None and off_subgroup is not None:
            break
    assert non_square is not None and off_subgroup is not None and pc.on_twist(off_subgroup)
    refused(_raw(pc, non_square.c, (0, 0), True), COMPRESSED, "x^3 + b is not a square")
    for compressed in (True, False):
        flags = COMPRESSED if compressed else 0
        rec = g2_record(pc, off_subgroup, compressed)
        refused(rec, flags | VALIDATE, "not in the subgroup")
        assert _decode(L, cid, rec, flags)[1] == off_subgroup                              # unchecked mode takes it, as ark's does
    # off the twist, uncompressed: only VALIDATE looks
    off = (pc.g2[0], pc.g2[1] + F([1]))
    refused(g2_record(pc, off, False), VALIDATE, "not on the curve")
    assert _decode(L, cid, g2_record(pc, off, False), 0)[1] == off


def _raw(pc, x, y, compressed):
    """a record from raw integers (no reduction), y's sign flag clear"""
    if pc.c.curve_id == 0:
        body = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big") + (b"" if compressed else y[1].to_bytes(48, "big") + y[0].to_bytes(48, "big")))
        body[0] |= 0x80 if compressed else 0
        return bytes(body)
    return x[0].to_bytes(32, "little") + x[1].to_bytes(32, "little") + (b"" if compressed else y[0].to_bytes(32, "little") + y[1].to_bytes(32, "little"))


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_batch_verify_challenge_is_the_transcripts(cid, K, L):
    """verifier.rs:203-215 by hand on the oracle's transcript"""
    c = pyref.CURVES[cid]
    us = [(0xC0FFEE + 977 * i) ** 9 % c.r for i in range(K)] if K != 2 else [0, c.r - 1]
    if K == 1:
        want = 1
    else:
        t = pyref_fs.StandardTranscript(c, b"batch verify")
        for u in us:
            t.append_field_elem(b"u", u)
        want = t.get_and_append_challenge(b"r")
    R = 1 << 256
    u_mont = np.array([l for u in us for l in _limbs(u * R % c.r, 4)], dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    assert L.mzk_batch_verify_challenge(cid, u_mont.ctypes.data, K, out.ctypes.data) == 0
    got = sum(int(out[j]) << (64 * j) for j in range(4))
    assert got < c.r and got * pow(R, -1, c.r) % c.r == want
    assert L.mzk_batch_verify_challenge(cid, u_mont.ctypes.data, 0, out.ctypes.data) == -1


def test_host_pairing_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_pairing_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "mpc-jellyfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "host_pairing_check.cpp")])
    out = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok") and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert sum("random tower cases checked" in l for l in out.stdout.splitlines()) == 2, out.stdout
