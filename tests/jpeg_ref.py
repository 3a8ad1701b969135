"""numpy restatement of a baseline JPEG decoder as libjpeg runs it by default -- what `PIL.Image.open(f).convert("RGB")` returns, bit
for bit: marker parser, bit reader, Huffman decode, dequantise + the "islow" integer IDCT (jidctint), "fancy" triangle chroma
upsampling (jdsample) and the 16-bit fixed-point YCbCr -> RGB conversion (jdcolor).  Plain and slow on purpose; tests hold it to
Pillow first and then hold `Dataset.parse_jpeg`, csrc/jpeg_entropy.h and csrc/jpeg.hip to it.

Scope (everything else parses to None): SOF0, 8-bit, one interleaved scan, 1 component or 3 components YCbCr with luma 1x1 / 2x1 /
2x2 and chroma 1x1, restart intervals, width and height 1 .. 4096."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])          # ZIGZAG[k] = natural (row-major) index of the k-th coefficient of the stream
MAX_DIM = 4096


class Corrupt(Exception):
    pass


def parse(data):
    """-> dict (see the keys at the bottom) or None for anything outside the scope."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return None
    pos = 2
    quant, huff = {}, {}
    frame = None
    restart = 0
    adobe = None
    while True:
        if pos + 2 > n or d[pos] != 0xFF:
            return None
        while pos < n and d[pos] == 0xFF:          # fill bytes
            pos += 1
        if pos >= n:
            return None
        m = d[pos]
        pos += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            return None                            # EOI before a scan
        if pos + 2 > n:
            return None
        ln = (d[pos] << 8) | d[pos + 1]
        if ln < 2 or pos + ln > n:
            return None
        seg = d[pos + 2:pos + ln]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0 or tq > 3 or q + 65 > len(seg):
                    return None
                nat = np.zeros(64, np.int32)
                nat[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                quant[tq] = nat
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    return None
                tc, th = seg[q] >> 4, seg[q] & 15
                bits = np.frombuffer(seg[q + 1:q + 17], np.uint8).copy()
                cnt = int(bits.sum())
                if tc > 1 or th > 1 or cnt > 256 or q + 17 + cnt > len(seg):
                    return None
                code = 0
                for l in range(16):                # a canonical code may not overflow its length
                    code += int(bits[l])
                    if code > (1 << (l + 1)):
                        return None
                    code <<= 1
                huff[(tc, th)] = (bits, np.frombuffer(seg[q + 17:q + 17 + cnt], np.uint8).copy())
                q += 17 + cnt
        elif m == 0xC0:
            if frame is not None or len(seg) < 6:
                return None
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8 or nc not in (1, 3) or len(seg) != 6 + 3 * nc or not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
                return None
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            frame = (h, w, comps)
        elif 0xC1 <= m <= 0xCF or m == 0xDC:       # every other SOF, arithmetic conditioning, DNL
            return None
        elif m == 0xDD:
            if len(seg) != 2:
                return None
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            break
        pos += ln
    if frame is None:
        return None
    h, w, comps = frame
    nc = len(comps)
    if len(seg) != 4 + 2 * nc or seg[0] != nc or seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
        return None
    sel = []
    for i in range(nc):
        if seg[1 + 2 * i] != comps[i][0]:
            return None
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if (0, td) not in huff or (1, ta) not in huff or comps[i][3] not in quant:
            return None
        sel.append((td, ta))
    if nc == 1:
        hs = vs = 1                                # a single component is never interleaved: its sampling factors are ignored
    else:
        if adobe == 0 or [c[0] for c in comps] == [82, 71, 66]:
            return None
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
    begin = pos + ln
    # entropy-coded data: up to the first marker that is neither a stuffed FF 00 nor a restart marker
    segs = [begin]
    p = begin
    end = None
    while p + 1 < n:
        if d[p] != 0xFF:
            p += 1
            continue
        nx = d[p + 1]
        if nx == 0:
            p += 2
        elif 0xD0 <= nx <= 0xD7:
            segs.append(p + 2)
            p += 2
        else:
            end = p
            break
    if end is None or d[end + 1] != 0xD9:          # cut short, a second scan, DNL, fill bytes: not walked
        return None
    mcus_w, mcus_h = -(-w // (8 * hs)), -(-h // (8 * vs))
    total = mcus_w * mcus_h
    if restart == 0:
        if len(segs) != 1:
            return None
        first = [0]
    else:
        if len(segs) > -(-total // restart):
            return None
        first = [k * restart for k in range(len(segs))]
    return dict(width=w, height=h, n_components=nc, h_samp=hs, v_samp=vs, restart_interval=restart,
                quant=[quant[c[3]] for c in comps],                       # natural order, per component
                dc=[huff[(0, s[0])] for s in sel], ac=[huff[(1, s[1])] for s in sel],      # (bits[16], huffval[]) per component
                quant_sel=[c[3] for c in comps], dc_sel=[s[0] for s in sel], ac_sel=[s[1] for s in sel],
                quant_tables=dict(quant), huff_tables=dict(huff),
                data_begin=begin, data_end=end, seg_offsets=segs, seg_first_mcu=first,
                mcus_w=mcus_w, mcus_h=mcus_h)


def _codebook(bits, vals):
    book, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(int(bits[l - 1])):
            book[(l, code)] = int(vals[k])
            code += 1
            k += 1
        code <<= 1
    return book


class _Bits:
    def __init__(self, raw):
        a = np.frombuffer(raw, np.uint8)
        keep = np.ones(a.size, bool)
        ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else []
        for i in ff:                               # FF 00 -> FF (inside a segment nothing else follows an FF)
            if keep[i]:
                keep[i + 1] = False
        self.bits = np.unpackbits(a[keep]).tolist()
        self.real = len(self.bits)
        self.bits += [0] * 64
        self.p = 0

    def symbol(self, book):
        code = 0
        for l in range(1, 17):
            if self.p >= len(self.bits):
                self.bits += [0] * 64              # zero bits past the end, as libjpeg supplies
            code = (code << 1) | self.bits[self.p]
            self.p += 1
            v = book.get((l, code))
            if v is not None:
                return v
        raise Corrupt("no such code")

    def receive_extend(self, s):
        if s == 0:
            return 0
        while self.p + s > len(self.bits):
            self.bits += [0] * 64
        x = 0
        for _ in range(s):
            x = (x << 1) | self.bits[self.p]
            self.p += 1
        return x if x >= (1 << (s - 1)) else x - (1 << s) + 1


def block_dims(hdr):
    """blocks (rows, cols) of each component's plane, padded to whole MCUs"""
    out = []
    for c in range(hdr["n_components"]):
        hs, vs = (hdr["h_samp"], hdr["v_samp"]) if c == 0 else (1, 1)
        out.append((hdr["mcus_h"] * vs, hdr["mcus_w"] * hs))
    return out


def decode_coefficients(data, hdr):
    """-> per component an int16 array (block_rows, block_cols, 64) in natural order, not dequantised.  Raises Corrupt."""
    d = bytes(data)
    dims = block_dims(hdr)
    coef = [np.zeros((bh, bw, 64), np.int16) for bh, bw in dims]
    dcb = [_codebook(*t) for t in hdr["dc"]]
    acb = [_codebook(*t) for t in hdr["ac"]]
    total = hdr["mcus_w"] * hdr["mcus_h"]
    ri = hdr["restart_interval"] or total
    segs = hdr["seg_offsets"]
    if len(segs) * ri < total:
        raise Corrupt("segments missing")
    for k, off in enumerate(segs):
        stop = segs[k + 1] - 2 if k + 1 < len(segs) else hdr["data_end"]
        br = _Bits(d[off:stop])
        pred = [0] * hdr["n_components"]
        for mcu in range(hdr["seg_first_mcu"][k], min(hdr["seg_first_mcu"][k] + ri, total)):
            my, mx = divmod(mcu, hdr["mcus_w"])
            for c in range(hdr["n_components"]):
                hs, vs = (hdr["h_samp"], hdr["v_samp"]) if c == 0 else (1, 1)
                for v in range(vs):
                    for hh in range(hs):
                        blk = coef[c][my * vs + v, mx * hs + hh]
                        s = br.symbol(dcb[c])
                        if s > 15:
                            raise Corrupt("dc size")
                        pred[c] += br.receive_extend(s)
                        blk[0] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                        kk = 1
                        while kk < 64:
                            rs = br.symbol(acb[c])
                            r, s = rs >> 4, rs & 15
                            if s:
                                kk += r
                                if kk > 63:
                                    raise Corrupt("coefficient index")
                                blk[ZIGZAG[kk]] = br.receive_extend(s)
                                kk += 1
                            elif r == 15:
                                kk += 16
                            else:
                                break
            if br.p > br.real:
                raise Corrupt("segment ends early")
    return coef


def _descale(x, n):
    """(x + half) >> n in a 32-bit register: sums and products before it are exact modulo 2^32, so wrapping once here is what 32-bit
    lanes hold.  Valid streams never wrap; a corrupt stream that still decodes may, and the device decoder is held to this too."""
    x = x + (1 << (n - 1))
    return (((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)) >> n


def _pass(v, shift):
    """one 1-D pass of jidctint's islow IDCT on v[..., 8], in int64 lanes"""
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (v[..., 0] + v[..., 4]) << 13
    tmp1 = (v[..., 0] - v[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                    tmp10 - tmp3], axis=-1)
    return _descale(out, shift)


def range_limit(x):
    """libjpeg's post-IDCT table lookup: clamp(x + 128) for |x| < 512, wrapping modulo 1024 beyond"""
    i = x & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def idct_planes(coef, hdr):
    """-> per component a uint8 plane (block_rows*8, block_cols*8)"""
    planes = []
    for c, cf in enumerate(coef):
        bh, bw = cf.shape[:2]
        v = cf.astype(np.int64).reshape(bh, bw, 8, 8) * hdr["quant"][c].astype(np.int64).reshape(8, 8)
        ws = _pass(v.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns
        px = range_limit(_pass(ws, 18))                               # rows
        planes.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes


def _h2_fancy(p):
    """h2v1 on the true plane p (rows, n): out (rows, 2n)"""
    p = p.astype(np.int32)
    prev = np.concatenate([p[:, :1], p[:, :-1]], 1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int32)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    return out.astype(np.uint8)


def _h2v2_fancy(p):
    p = p.astype(np.int32)
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int32)
    for v, other in ((0, up), (1, dn)):
        s = 3 * p + other
        last = np.concatenate([s[:, :1], s[:, :-1]], 1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[v::2, 0::2] = (3 * s + last + 8) >> 4
        out[v::2, 1::2] = (3 * s + nxt + 7) >> 4
    return out.astype(np.uint8)


def upsample(plane, hdr):
    """a chroma plane -> at least (height, width) samples.  libjpeg picks the triangle filter only where the down-sampled
    plane is more than two samples wide; narrower planes are replicated."""
    h, w, hs, vs = hdr["height"], hdr["width"], hdr["h_samp"], hdr["v_samp"]
    if hs == 1:
        return plane[:h, :w]
    dw, dh = -(-w // 2), (-(-h // 2) if vs == 2 else h)
    true = plane[:dh, :dw]
    if dw <= 2:
        out = np.repeat(true, 2, axis=1)
        return np.repeat(out, 2, axis=0) if vs == 2 else out
    return _h2v2_fancy(true) if vs == 2 else _h2_fancy(true)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """-> (height, width, 3) uint8 RGB, or None when the stream is outside the scope"""
    hdr = parse(data)
    if hdr is None:
        return None
    planes = idct_planes(decode_coefficients(data, hdr), hdr)
    h, w = hdr["height"], hdr["width"]
    if hdr["n_components"] == 1:
        return np.repeat(planes[0][:h, :w, None], 3, axis=2)
    cb, cr = upsample(planes[1], hdr)[:h, :w], upsample(planes[2], hdr)[:h, :w]
    return ycc_to_rgb(planes[0][:h, :w], cb, cr)


# ---- the fixtures every JPEG test shares: encoded by Pillow from seeded arrays -------------------------------------------------
SIZES = [(1, 1), (8, 8), (13, 17), (31, 33), (48, 64), (75, 97)]
MODES = [("q30_420", dict(quality=30, subsampling="4:2:0")),
         ("q75_422", dict(quality=75, subsampling="4:2:2")),
         ("q95_444", dict(quality=95, subsampling="4:4:4")),
         ("q100_420_opt", dict(quality=100, subsampling="4:2:0", optimize=True)),
         ("q75_420_rstblk1", dict(quality=75, subsampling="4:2:0", restart_marker_blocks=1)),
         ("q90_420_rstrow1", dict(quality=90, subsampling="4:2:0", restart_marker_rows=1))]


def encode(arr, **kw):
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG", **kw)
    return f.getvalue()


def pillow(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_cache = {}


def matrix():
    """[(name, (h, w), bytes)]: the base matrix, then the extra cases"""
    if "m" not in _cache:
        rng = np.random.default_rng(1)
        out = []
        for h, w in SIZES:
            px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            for name, kw in MODES:
                out.append((f"{h}x{w}_{name}", (h, w), encode(px, **kw)))
        out.append(("31x33_gray", (31, 33), encode(rng.integers(0, 256, (31, 33), dtype=np.uint8), quality=80)))
        out.append(("48x64_rstblk3", (48, 64), encode(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), quality=75,
                                                      subsampling="4:2:0", restart_marker_blocks=3)))
        yy, xx = np.mgrid[0:75, 0:97]
        smooth = np.stack([127.5 + 127.5 * np.sin(xx / 9.0 + yy / 17.0), 127.5 + 127.5 * np.cos(xx / 23.0),
                           127.5 + 127.5 * np.sin(yy / 11.0)], -1).astype(np.uint8)
        out.append(("75x97_smooth", (75, 97), encode(smooth, quality=75, subsampling="4:2:0")))
        _cache["m"] = out
    return _cache["m"]


def corrupt_streams():
    """[(name, bytes)]: every base-matrix stream of size (31, 33) with its entropy-coded data cut at 25 / 50 / 75 % (the EOI marker
    put back, so the stream still parses), and with 16 seeded single-bit flips in the entropy-coded data (a flip that would make or
    break a marker is drawn again, so the segment table stays that of the original)."""
    if "c" not in _cache:
        out = []
        rng = np.random.default_rng(7)
        for name, hw, data in matrix()[:len(SIZES) * len(MODES)]:
            if hw != (31, 33):
                continue
            hdr = parse(data)
            b, e = hdr["data_begin"], hdr["data_end"]
            for pct in (25, 50, 75):
                cut = b + (e - b) * pct // 100
                while data[cut - 1] == 0xFF:       # never end on half of a marker or of a stuffed pair
                    cut -= 1
                out.append((f"{name}_cut{pct}", data[:cut] + b"\xff\xd9"))
            buf = bytearray(data)
            done = 0
            while done < 16:
                i, bit = int(rng.integers(b, e)), int(rng.integers(0, 8))
                trial = buf[i] ^ (1 << bit)
                if 0xFF in (buf[i], trial) or buf[i - 1] == 0xFF:
                    continue
                buf[i] = trial
                done += 1
            out.append((f"{name}_flip16", bytes(buf)))
        _cache["c"] = out
    return _cache["c"]
