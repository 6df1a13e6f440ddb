"""MJPEG input, restated in numpy: a baseline JPEG decoder -- marker parser, bit-serial Huffman decode, dequantisation,
the IJG accurate integer inverse DCT in wrapping int32, the way to the coded NV12 surfaces -- and a small baseline JPEG writer, so that no test
depends on an installed codec.  The writer returns the exact coefficients it coded."""
import numpy as np

from tests import cscref

FMT_I420, FMT_Y42B, FMT_Y444 = 1, 4, 5
SAMPLING = {"grey": (1, 1, 1), "420": (3, 2, 2), "422": (3, 2, 1), "444": (3, 1, 1)}  # components, hs, vs


def _zigzag():
    order, (r, c) = [], (0, 0)
    for _ in range(64):
        order.append(r * 8 + c)
        if (r + c) % 2 == 0:
            if c == 7: r += 1
            elif r == 0: c += 1
            else: r, c = r - 1, c + 1
        else:
            if r == 7: c += 1
            elif c == 0: r += 1
            else: r, c = r + 1, c - 1
    return np.array(order)


NATURAL = _zigzag()  # NATURAL[k]: the row-major position of zigzag index k

# T.81 Annex K.3 typical Huffman tables: (16 counts, symbols)
STD_DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
STD_AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
    "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa".replace(" ", ""))))
STD_TABLES = {(0, 0): STD_DC_L, (0, 1): STD_DC_C, (1, 0): STD_AC_L, (1, 1): STD_AC_C}  # (class, index)

# T.81 Annex K.1 quantisation tables, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def scaled_q(q, percent):
    return np.clip((q * percent + 50) // 100, 1, 255)


def generated_tables(seed):
    """A non-typical Huffman table set with codes of up to 16 bits: all 12 DC and all 162 AC symbols in a seeded order"""
    rng = np.random.default_rng(seed)
    dc_bits = [0, 1, 1, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1]
    ac_bits = [0, 1, 1, 1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 24, 20, 20]
    ac_syms = STD_AC_L[1]
    out = {}
    for i in range(2):
        out[(0, i)] = (dc_bits, [int(v) for v in rng.permutation(12)])
        out[(1, i)] = (ac_bits, [int(v) for v in rng.permutation(ac_syms)])
    return out


def huff_codes(bits, vals):
    """symbol -> (code, length)"""
    codes, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            codes[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return codes


# ------------------------------------------------------------------------------------------------ the writer
def _dct_matrix():
    m = np.zeros((8, 8))
    for u in range(8):
        for x in range(8):
            m[u, x] = (np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return m


_DCT = _dct_matrix()


def _pad_edge(p, hh, ww):
    p = np.asarray(p)
    return np.pad(p, ((0, hh - p.shape[0]), (0, ww - p.shape[1])), mode="edge")


def quantise(planes, sampling, qts):
    """planes (Y[, U, V] at their sampled sizes) -> per component the int16 blocks (block rows, blocks per row, 8, 8) of the MCU-padded plane"""
    nc, hs, vs = SAMPLING[sampling]
    h, w = planes[0].shape
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    out = []
    for c in range(nc):
        bw, bh = mcux * (1 if c else hs), mcuy * (1 if c else vs)
        p = _pad_edge(planes[c], bh * 8, bw * 8).astype(np.float64) - 128.0
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        co = _DCT @ blocks @ _DCT.T
        q = np.asarray(qts[1 if c else 0], np.float64).reshape(8, 8)
        lv = np.rint(co / q).astype(np.int64)
        lv[..., 1:, :] = np.clip(lv[..., 1:, :], -1023, 1023)
        lv[..., 0, 1:] = np.clip(lv[..., 0, 1:], -1023, 1023)
        out.append(lv.astype(np.int16))
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def encode_coefs(coefs, w, h, sampling, qts=(Q_LUMA, Q_CHROMA), tables=None, dri=0, dht=True, sof_marker=0xC0, precision=8, luma_hv=None, pq=0,
                 scan_components=None, extra_component=False, app=True, split_tables=False, fill=False):
    """Coefficient blocks (as quantise() returns them) -> a JPEG byte stream.  tables: {(class, index): (bits, vals)} (default: the typical ones; dht False
    leaves the DHT segment out).  The arguments from sof_marker on write streams the decoder must refuse (the entropy-coded data then means nothing)."""
    nc, hs, vs = SAMPLING[sampling]
    tables = tables or STD_TABLES
    out = bytearray(b"\xff\xd8")
    if app:
        out += _seg(0xE0, b"AVI1\0\0\0\0\0\0\0\0\0\0") + _seg(0xFE, b"mi355 test picture")
    dqt = bytearray()
    for i in range(2 if nc == 3 else 1):
        zz = np.asarray(qts[i]).ravel()[NATURAL]
        body = bytes([(pq << 4) | i]) + (b"".join(int(v).to_bytes(2, "big") for v in zz) if pq else bytes(int(v) for v in zz))
        if split_tables:
            out += _seg(0xDB, body)
        else:
            dqt += body
    if dqt:
        out += _seg(0xDB, dqt)  # several tables in one segment
    ncomp = nc + (1 if extra_component else 0)
    sof = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        hv = (luma_hv if luma_hv is not None else (hs << 4) | vs) if c == 0 else 0x11
        sof += bytes([c + 1, hv, 1 if c else 0])
    if fill:
        out += b"\xff\xff"  # fill bytes in front of a marker
    out += _seg(sof_marker, sof)
    if dht:
        body = bytearray()
        for (cl, i), (bits, vals) in sorted(tables.items()):
            if i == 1 and nc == 1:
                continue
            b = bytes([(cl << 4) | i]) + bytes(bits) + bytes(vals)
            if split_tables:
                out += _seg(0xC4, b)
            else:
                body += b
        if body:
            out += _seg(0xC4, body)
    if dri:
        out += _seg(0xDD, dri.to_bytes(2, "big"))
    ns = scan_components or ncomp
    sos = bytes([ns])
    for c in range(ns):
        sos += bytes([c + 1, 0x11 if c else 0x00])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    codes = {k: huff_codes(*v) for k, v in tables.items()}
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    bits, pred, n = _Bits(), [0] * nc, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if dri and n and n % dri == 0:
                bits.flush()
                out += bits.out + bytes([0xFF, 0xD0 + ((n // dri - 1) & 7)])
                bits, pred = _Bits(), [0] * nc
            n += 1
            for c in range(nc):
                hc, vc = (hs, vs) if c == 0 else (1, 1)
                dc, ac = codes[(0, 1 if c else 0)], codes[(1, 1 if c else 0)]
                for j in range(vc):
                    for i in range(hc):
                        zz = coefs[c][my * vc + j, mx * hc + i].ravel()[NATURAL].astype(np.int64)
                        d = int(zz[0]) - pred[c]
                        pred[c] = int(zz[0])
                        s = _size(d)
                        bits.put(*dc[s])
                        if s:
                            bits.put(d if d > 0 else d + (1 << s) - 1, s)
                        run = 0
                        nz = np.flatnonzero(zz[1:])
                        last = int(nz[-1]) + 1 if nz.size else 0
                        for k in range(1, last + 1):
                            v = int(zz[k])
                            if v == 0:
                                run += 1
                                continue
                            while run > 15:
                                bits.put(*ac[0xF0])
                                run -= 16
                            s = _size(v)
                            bits.put(*ac[(run << 4) | s])
                            bits.put(v if v > 0 else v + (1 << s) - 1, s)
                            run = 0
                        if last < 63:
                            bits.put(*ac[0x00])
    bits.flush()
    out += bits.out + b"\xff\xd9"
    return bytes(out)


def subsample(y, u, v, sampling):
    """full-size planes -> the planes a picture of this sampling carries (box means)"""
    if sampling == "grey":
        return [y]
    if sampling == "444":
        return [y, u, v]
    u, v = ((c[:, 0::2].astype(np.uint16) + c[:, 1::2] + 1) >> 1 for c in (u, v))
    if sampling == "420":
        u, v = ((c[0::2] + c[1::2] + 1) >> 1 for c in (u, v))
    return [y, u.astype(np.uint8), v.astype(np.uint8)]


def write_jpeg(planes, sampling, qts=(Q_LUMA, Q_CHROMA), **kw):
    """planes at their sampled sizes -> (bytes, coefficient blocks)"""
    h, w = planes[0].shape
    coefs = quantise(planes, sampling, qts)
    return encode_coefs(coefs, w, h, sampling, qts, **kw), coefs


def picture(w, h, seed, noise=40):
    """a seeded test picture: gradients, an edge and noise, full size Y, U, V"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = 128 + 90 * np.sin(xx / 5.0 + seed) * np.cos(yy / 7.0) + rng.integers(-noise, noise + 1, (h, w))
    y[:, w // 3:w // 3 + 2] = 255
    u = 128 + 100 * np.sin((xx + yy) / 9.0) + rng.integers(-noise, noise + 1, (h, w))
    v = 128 + 100 * np.cos((xx - yy) / 6.0) + rng.integers(-noise, noise + 1, (h, w))
    return [np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v)]


# ------------------------------------------------------------------------------------------------ the decoding rule
class Refused(ValueError):
    pass


def parse(data):
    """-> dict(width, height, components, hs, vs, restart_interval, has_dht, qt [per component, natural order], tables {(class, index): (bits, vals)},
    td, ta, scan); Refused for anything but the accepted streams"""
    d = bytes(data)
    if len(d) < 4 or d[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    pos, hdr, qts, tabs, sof = 2, {"restart_interval": 0, "has_dht": 0}, {}, {}, None
    while True:
        if pos >= len(d) or d[pos] != 0xFF:
            raise Refused("no marker")
        while pos < len(d) and d[pos] == 0xFF:
            pos += 1
        if pos >= len(d):
            raise Refused("end")
        m = d[pos]
        pos += 1
        if m in (0, 1) or 0xD0 <= m <= 0xD9:
            raise Refused("marker %02x" % m)
        if pos + 2 > len(d):
            raise Refused("end")
        L = int.from_bytes(d[pos:pos + 2], "big")
        if L < 2 or pos + L > len(d):
            raise Refused("length")
        seg = d[pos + 2:pos + L]
        pos += L
        if m in (0xC0, 0xC1):
            if sof is not None or len(seg) < 6 or seg[0] != 8:
                raise Refused("SOF")
            nf = seg[5]
            if nf not in (1, 3) or len(seg) != 6 + 3 * nf:
                raise Refused("components")
            sof = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(nf)]
            hdr.update(height=int.from_bytes(seg[1:3], "big"), width=int.from_bytes(seg[3:5], "big"), components=nf, hs=1, vs=1)
            if hdr["width"] < 1 or hdr["height"] < 1 or any(c[2] > 3 for c in sof):
                raise Refused("SOF")
            if nf == 3:
                if sof[1][1] != 0x11 or sof[2][1] != 0x11 or sof[0][1] not in (0x22, 0x21, 0x11):
                    raise Refused("sampling")
                hdr["hs"], hdr["vs"] = sof[0][1] >> 4, sof[0][1] & 15
        elif 0xC2 <= m <= 0xCF and m != 0xC4:
            raise Refused("SOF%d" % (m - 0xC0))
        elif m == 0xC4:
            while seg:
                if len(seg) < 17 or seg[0] >> 4 > 1 or seg[0] & 15 > 3:
                    raise Refused("DHT")
                n = sum(seg[1:17])
                if n > 256 or len(seg) < 17 + n:
                    raise Refused("DHT")
                tabs[(seg[0] >> 4, seg[0] & 15)] = (list(seg[1:17]), list(seg[17:17 + n]))
                hdr["has_dht"] = 1
                seg = seg[17 + n:]
        elif m == 0xDB:
            while seg:
                if len(seg) < 65 or seg[0] >> 4 or seg[0] & 15 > 3:
                    raise Refused("DQT")
                q = np.zeros(64, np.uint16)
                q[NATURAL] = list(seg[1:65])
                qts[seg[0] & 15] = q
                seg = seg[65:]
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused("DRI")
            hdr["restart_interval"] = int.from_bytes(seg, "big")
        elif m == 0xDA:
            if sof is None or len(seg) < 1 or seg[0] != hdr["components"] or len(seg) != 1 + 2 * seg[0] + 3:
                raise Refused("SOS")
            td, ta = [], []
            for c in range(seg[0]):
                if seg[1 + 2 * c] != sof[c][0] or seg[2 + 2 * c] >> 4 > 3 or seg[2 + 2 * c] & 15 > 3:
                    raise Refused("SOS")
                td.append(seg[2 + 2 * c] >> 4)
                ta.append(seg[2 + 2 * c] & 15)
            if tuple(seg[-3:]) != (0, 63, 0):
                raise Refused("spectral selection")
            break
    for c in range(hdr["components"]):
        if sof[c][2] not in qts:
            raise Refused("no quantisation table")
        if hdr["has_dht"]:
            if (0, td[c]) not in tabs or (1, ta[c]) not in tabs:
                raise Refused("no Huffman table")
        elif td[c] > 1 or ta[c] > 1:
            raise Refused("no Huffman table")
    if not hdr["has_dht"]:
        tabs = STD_TABLES
    hdr.update(qt=[qts[sof[c][2]] for c in range(hdr["components"])], tables=tabs, td=td, ta=ta, scan=pos)
    return hdr


def layout(hdr):
    mcux, mcuy = -(-hdr["width"] // (8 * hdr["hs"])), -(-hdr["height"] // (8 * hdr["vs"]))
    return [(mcux * (1 if c else hdr["hs"]), mcuy * (1 if c else hdr["vs"])) for c in range(hdr["components"])]


class _Reader:
    """bits of the entropy-coded segment up to the next marker"""

    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def bit(self):
        if self.n == 0:
            d, p = self.d, self.pos
            if p < len(d) and d[p] != 0xFF:
                self.acc, self.pos = d[p], p + 1
            elif p + 1 < len(d) and d[p + 1] == 0:
                self.acc, self.pos = 0xFF, p + 2
            else:
                raise Refused("data ends")
            self.n = 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, lookup):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            s = lookup.get((code, l))
            if s is not None:
                return s
        raise Refused("undefined code")

    def extend(self, s):
        v = self.bits(s)
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy_decode(data):
    """-> (header dict, [per component int16 (block rows, blocks per row, 8, 8)], uint16 qt (3, 64)); Refused for a corrupt picture"""
    hdr = parse(data)
    d = bytes(data)
    look = {}
    for key, (bits, vals) in hdr["tables"].items():
        code, k, lk = 0, 0, {}
        for l in range(1, 17):
            if code + bits[l - 1] > 1 << l:
                raise Refused("Huffman table")
            for _ in range(bits[l - 1]):
                lk[(code, l)] = vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        look[key] = lk
    nc, hs, vs, ri = hdr["components"], hdr["hs"], hdr["vs"], hdr["restart_interval"]
    lay = layout(hdr)
    coefs = [np.zeros((bh, bw, 64), np.int16) for bw, bh in lay]
    r, pred, n = _Reader(d, hdr["scan"]), [0] * nc, 0
    for my in range(lay[0][1] // vs):
        for mx in range(lay[0][0] // hs):
            if ri and n and n % ri == 0:
                p = r.pos
                if p >= len(d) or d[p] != 0xFF:
                    raise Refused("no RST")
                while p < len(d) and d[p] == 0xFF:
                    p += 1
                if p >= len(d) or d[p] != 0xD0 + ((n // ri - 1) & 7):
                    raise Refused("RST out of order")
                r, pred = _Reader(d, p + 1), [0] * nc
            n += 1
            for c in range(nc):
                hc, vc = (hs, vs) if c == 0 else (1, 1)
                dc, ac = look[(0, hdr["td"][c])], look[(1, hdr["ta"][c])]
                for j in range(vc):
                    for i in range(hc):
                        blk = coefs[c][my * vc + j, mx * hc + i]
                        s = r.symbol(dc)
                        if s > 11:
                            raise Refused("DC size")
                        pred[c] += r.extend(s) if s else 0
                        if not -32768 <= pred[c] <= 32767:
                            raise Refused("DC range")
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = r.symbol(ac)
                            run, s = rs >> 4, rs & 15
                            if s == 0:
                                if run != 15:
                                    break
                                k += 16
                                if k > 64:
                                    raise Refused("run")
                                continue
                            if s > 10:
                                raise Refused("AC size")
                            k += run
                            if k > 63:
                                raise Refused("run")
                            blk[NATURAL[k]] = r.extend(s)
                            k += 1
    qt = np.zeros((3, 64), np.uint16)
    for c in range(nc):
        qt[c] = hdr["qt"][c]
    return hdr, [c.reshape(c.shape[0], c.shape[1], 8, 8) for c in coefs], qt


def _pass(d, shift):
    """one 8-point pass of jidctint along the last axis, int32 with wrap-around"""
    i32 = np.int32
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * i32(4433)
    t2, t3 = z1 + d[6] * i32(-15137), z1 + d[2] * i32(6270)
    t0, t1 = (d[0] + d[4]) << i32(13), (d[0] - d[4]) << i32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * i32(9633)
    o0, o1, o2, o3 = o0 * i32(2446), o1 * i32(16819), o2 * i32(25172), o3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    rnd = i32(1 << (shift - 1))
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(v + rnd) >> i32(shift) for v in out], axis=-1)


def idct(coef, q):
    """blocks (..., 8, 8) int16 and a quantisation table (64 or 8 x 8) -> samples (..., 8, 8) uint8: the device's arithmetic, wrap-around included"""
    with np.errstate(over="ignore"):
        d = coef.astype(np.int32) * np.asarray(q).reshape(8, 8).astype(np.int32)
        ws = _pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns first
        x = _pass(ws, 18)
        return np.clip(x + np.int32(128), 0, 255).astype(np.uint8)


def planes_from_coefs(coefs, qt, w, h, hs, vs):
    """-> the visible planes: Y (h, w) and, with three components, U and V at their sampled size"""
    out = []
    for c, co in enumerate(coefs):
        bh, bw = co.shape[:2]
        p = idct(co, qt[c]).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(np.ascontiguousarray(p[:h // (vs if c else 1), :w // (hs if c else 1)]))
    return out


def decode(data):
    """-> (fmt, planes): FMT_I420 / FMT_Y42B / FMT_Y444 and Y, U, V; a grey picture comes back as I420 with chroma 128"""
    hdr, coefs, qt = entropy_decode(data)
    w, h = hdr["width"], hdr["height"]
    if (w | h) & 1:
        raise Refused("odd size")
    planes = planes_from_coefs(coefs, qt, w, h, hdr["hs"], hdr["vs"])
    return planar(planes, w, h, hdr["hs"], hdr["vs"])


def planar(planes, w, h, hs, vs):
    if len(planes) == 1:
        return FMT_I420, [planes[0], np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)]
    return {(2, 2): FMT_I420, (2, 1): FMT_Y42B, (1, 1): FMT_Y444}[(hs, vs)], planes


def surfaces(fmt, planes, w, h):
    """the coded-size NV12 surfaces of the planar picture: what mi355enc_stage_csc makes of it"""
    return cscref.to_nv12(fmt, planes, w, h)
