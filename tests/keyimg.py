"""Test-side builder of serialized ProvingKey / VerifyingKey images (ark-serialize 0.4, derive order: include/mzk.h, mzk_key_layout), from
oracle/pyref_fs.fr_bytes / g1_bytes / vec_bytes and the format alone -- nothing of the product is used.  While concatenating it records
where every field starts: `spans` (name, first byte, end) for every prefix, tag and body in image order -- the names are the ones
mzk_last_error() uses -- and `layout`, the offsets and counts mzk_key_layout must report."""
import struct

import pyref_fs

TABLE_POLYS = ("range_table_poly", "key_table_poly", "table_dom_sep_poly", "q_dom_sep_poly")


def g1_record(pc, pt, compress=True) -> bytes:
    """Affine<G1>: pyref_fs.g1_bytes when compressed; uncompressed x || y (BLS12-381 big-endian, byte 0: 0x40 infinity; BN254 little-endian,
    byte 63: 0x80 y is the larger, 0x40 infinity)."""
    if compress:
        return pyref_fs.g1_bytes(pc, pt)
    if pc.curve_id == 0:
        return bytes([0x40]) + bytes(95) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")
    if pt is None:
        return bytes(63) + bytes([0x40])
    out = bytearray(pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"))
    if pt[1] > pc.q - pt[1]:
        out[63] |= 0x80
    return bytes(out)


def g2_bytes(pc, compress=True) -> int:
    return (96 if pc.curve_id == 0 else 64) * (1 if compress else 2)


def strip(coeffs):
    """DensePolynomial::from_coefficients_vec: trailing zeros go"""
    coeffs = list(coeffs)
    while coeffs and coeffs[-1] == 0:
        coeffs.pop()
    return coeffs


class Image:
    def __init__(self):
        self.data, self.spans, self.layout = bytearray(), [], {}

    def put(self, name, b):
        self.spans.append((name, len(self.data), len(self.data) + len(b)))
        self.data += b

    def u64(self, name, v):
        self.put(name, struct.pack("<Q", v))

    def field_at(self, cut):
        """the field a cut after `cut` bytes falls in: the first non-empty span that ends beyond it"""
        return next(name for name, a, b in self.spans if b > cut and b > a)


def _put_vk(im, pc, compress, vk):
    L, enc = im.layout, (lambda pt: g1_record(pc, pt, compress))
    L["vk_off"] = len(im.data)
    im.u64("vk.domain_size", vk["domain_size"])
    im.u64("vk.num_inputs", vk["num_inputs"])
    for key in ("sigma_comms", "selector_comms"):
        im.u64(f"vk.{key}.len", len(vk[key]))
        L[key + "_off"] = len(im.data)
        im.put(f"vk.{key}", b"".join(enc(p) for p in vk[key]))
    im.u64("vk.k.len", len(vk["k"]))
    L["k_off"] = len(im.data)
    im.put("vk.k", b"".join(pyref_fs.fr_bytes(pc, x) for x in vk["k"]))
    for key in ("g", "h", "beta_h"):
        L[key + "_off"] = len(im.data)
        im.put("vk.open_key." + key, enc(vk["g"]) if key == "g" else vk[key])
    im.put("vk.is_merged", bytes([int(vk.get("is_merged", False))]))
    pl = vk.get("plookup_comms")
    im.put("vk.plookup_vk", bytes([0 if pl is None else 1]))
    if pl is not None:
        L["plookup_comms_off"] = len(im.data)
        im.put("vk.plookup_vk", b"".join(enc(p) for p in pl))
    L["vk_len"] = len(im.data) - L["vk_off"]


def vk_image(pc, compress, vk) -> Image:
    im = Image()
    _put_vk(im, pc, compress, vk)
    im.layout["total_len"] = len(im.data)
    return im


def pk_image(pc, compress, sigmas, selectors, commit_key, vk, tables=None) -> Image:
    """sigmas / selectors / tables: coefficient lists (canonical integers, written as given: strip() them first for what ark writes);
    commit_key: points; vk: dict(domain_size, num_inputs, sigma_comms, selector_comms, k, g, h, beta_h[, is_merged, plookup_comms]) with
    points as (x, y) / None and h, beta_h as bytes."""
    im = Image()
    L = im.layout

    def poly(name, coeffs):
        im.u64(name + ".len", len(coeffs))
        off = len(im.data)
        im.put(name, b"".join(pyref_fs.fr_bytes(pc, x) for x in coeffs))
        return off, len(coeffs)

    for key, polys in (("sigmas", sigmas), ("selectors", selectors)):
        im.u64(key + ".len", len(polys))
        L[key] = [poly(f"{key}[{i}]", p) for i, p in enumerate(polys)]
    im.u64("commit_key.len", len(commit_key))
    L["commit_key_off"], L["commit_key_count"] = len(im.data), len(commit_key)
    im.put("commit_key", b"".join(g1_record(pc, p, compress) for p in commit_key))
    _put_vk(im, pc, compress, vk)
    im.put("plookup_pk", bytes([0 if tables is None else 1]))
    L["tables"] = [] if tables is None else [poly("plookup_pk." + name, p) for name, p in zip(TABLE_POLYS, tables)]
    L["total_len"] = len(im.data)
    return im
