"""Progressive JPEG (SOF2) fixtures: a writer from known coefficients under an arbitrary scan script, and a model decoder.

Both are written from ITU-T T.81 Annex G (encoder procedures G.1.2.1 - G.1.2.3 with buffered correction bits and EOBRUN; decoder
Figure G.7) and Annex K.2 (optimised Huffman tables, one fresh set per scan, as optimising encoders write them).  Test infrastructure,
not product code: the model decoder is deliberately bit-at-a-time and shares nothing with the library.

Planes are what the library's entropy decoders deliver: per component an int16 array [blocks][64], blocks in MCU order (h x v blocks of
the first component per MCU, one of each chroma component), natural order inside a block.
"""
import numpy as np

from jpeg_entropy import ZZ

def geometry(width, height, h, v):
    """(mcu_cols, mcu_rows)"""
    return -(-width // (8 * h)), -(-height // (8 * v))


def comp_grid(width, height, h, v, c):
    """blocks per row and rows of component c's own grid: ceil(ceil(W h_c / h_max) / 8) x ceil(ceil(H v_c / v_max) / 8)"""
    hc, vc = (h, v) if c == 0 else (1, 1)
    return -(-(-(-width * hc // h)) // 8), -(-(-(-height * vc // v)) // 8)


def block_index(mcu_cols, h, v, c, bx, by):
    hc, vc = (h, v) if c == 0 else (1, 1)
    return ((by // vc) * mcu_cols + bx // hc) * (hc * vc) + (by % vc) * hc + bx % hc


def scan_units(width, height, h, v, comps):
    """per unit of a scan the list of (component, block index): MCUs of an interleaved scan, the component's own grid otherwise"""
    mcu_cols, mcu_rows = geometry(width, height, h, v)
    if len(comps) > 1:
        units = []
        for m in range(mcu_cols * mcu_rows):
            units.append([(c, m * (h * v if c == 0 else 1) + q) for c in comps for q in range(h * v if c == 0 else 1)])
        return units
    c = comps[0]
    bw, bh = comp_grid(width, height, h, v, c)
    return [[(c, block_index(mcu_cols, h, v, c, bx, by))] for by in range(bh) for bx in range(bw)]


# ---------------------------------------------------------------- Huffman tables (K.2) ----
def optimal_table(freq):
    """freq: {symbol: count} -> (counts[16], symbols) of a code of at most 16 bits without an all-ones code word (K.2, Figures K.1 - K.4)"""
    f = [0] * 257
    for s, n in freq.items():
        f[s] = n
    f[256] = 1
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 60
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 60
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 64
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(63, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                  # the reserved all-ones code word
    symbols = [s for length in range(1, 64) for s in range(256) if codesize[s] == length]
    return bits[1:17], symbols


def code_book(counts, symbols):
    """{symbol: (code, length)}"""
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            book[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return book


# ---------------------------------------------------------------- the writer ----
class _Tokens:
    """a scan's symbols and raw bits in order, cut into restart intervals; Huffman symbols are ('s', table, symbol)"""

    def __init__(self):
        self.intervals = [[]]

    def sym(self, table, symbol):
        self.intervals[-1].append(("s", table, symbol))

    def bits(self, value, n):
        if n:
            self.intervals[-1].append(("b", value & ((1 << n) - 1), n))

    def restart(self):
        self.intervals.append([])


def _nbits(v):
    return int(v).bit_length()


def _encode_scan(tok, units, planes, ss, se, ah, al, restart, comps):
    """G.1.2: tokens of one scan.  Tables are named by the scan component's position (DC) or 0 (AC)."""
    pos = {c: k for k, c in enumerate(comps)}
    pred = {c: 0 for c in comps}
    state = dict(eobrun=0, be=[])                 # be: correction bits buffered behind the pending EOBRUN

    def emit_eobrun():
        if state["eobrun"]:
            n = _nbits(state["eobrun"]) - 1
            tok.sym(0, n << 4)
            tok.bits(state["eobrun"], n)
            state["eobrun"] = 0
        for b in state["be"]:
            tok.bits(b, 1)
        state["be"] = []

    for u, unit in enumerate(units):
        if restart and u and u % restart == 0:
            emit_eobrun()
            tok.restart()
            pred = {c: 0 for c in comps}
        for c, bi in unit:
            blk = planes[c][bi]
            if ss == 0:
                if ah:
                    tok.bits((int(blk[0]) >> al) & 1, 1)
                    continue
                t = int(blk[0]) >> al             # the DC point transform is an arithmetic shift
                d = t - pred[c]
                pred[c] = t
                n = _nbits(abs(d))
                tok.sym(pos[c], n)
                tok.bits(d if d >= 0 else d - 1, n)
                continue
            band = [int(blk[ZZ[k]]) for k in range(ss, se + 1)]
            mags = [abs(x) >> al for x in band]   # the AC point transform divides the magnitude
            if not ah:
                r = 0
                for x, m in zip(band, mags):
                    if m == 0:
                        r += 1
                        continue
                    emit_eobrun()
                    while r > 15:
                        tok.sym(0, 0xF0)
                        r -= 16
                    n = _nbits(m)
                    tok.sym(0, (r << 4) | n)
                    tok.bits(m if x >= 0 else ~m, n)
                    r = 0
                if r:
                    state["eobrun"] += 1
                    if state["eobrun"] == 0x7FFF:
                        emit_eobrun()
                continue
            # G.1.2.3: refinement with correction bits buffered until the symbol they follow is known
            eob = max([k for k, m in enumerate(mags) if m == 1], default=-1)
            r, br = 0, []
            for k, (x, m) in enumerate(zip(band, mags)):
                if m == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    tok.sym(0, 0xF0)
                    r -= 16
                    for b in br:
                        tok.bits(b, 1)
                    br = []
                if m > 1:
                    br.append(m & 1)
                    continue
                emit_eobrun()
                tok.sym(0, (r << 4) | 1)
                tok.bits(0 if x < 0 else 1, 1)
                for b in br:
                    tok.bits(b, 1)
                br = []
                r = 0
            if r or br:
                state["eobrun"] += 1
                state["be"] += br
                if state["eobrun"] == 0x7FFF or len(state["be"]) > 1000 - 64 + 1:
                    emit_eobrun()
    emit_eobrun()


def _pack(interval, books):
    out, acc, n = bytearray(), 0, 0
    for t in interval:
        if t[0] == "s":
            code, length = books[t[1]][t[2]]
        else:
            code, length = t[1], t[2]
        acc = (acc << length) | code
        n += length
        while n >= 8:
            n -= 8
            b = (acc >> n) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc &= (1 << n) - 1
    if n:
        b = ((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 0xFF
        out.append(b)
        if b == 0xFF:
            out.append(0)
    return bytes(out)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def encode_progressive(width, height, h, v, coef, quant, script, restart=0, ncomp=None, eoi=True, raw_scan_hook=None, token_hook=None):
    """A SOF2 file from known coefficients.
    coef     per component an int16 array [blocks][64] (MCU order, natural order inside a block)
    quant    [64] or [ncomp][64] natural-order quantisers; table 0 for the first component, 1 for the others
    script   list of (components, Ss, Se, Ah, Al), components a tuple of frame indices
    restart  DRI in units of the scan (MCUs, or blocks of a non-interleaved scan); 0 = none
    raw_scan_hook(i, header_payload, entropy_bytes) -> (header_payload, entropy_bytes): to damage scan i on purpose
    token_hook(i, intervals): sees scan i's symbols and raw bits as they were emitted, per restart interval"""
    ncomp = ncomp or len(coef)
    quant = np.asarray(quant, dtype=np.uint16).reshape(-1, 64)
    out = bytearray(b"\xff\xd8")
    for t in range(min(len(quant), 2 if ncomp > 1 else 1)):
        out += _seg(0xDB, bytes([t]) + bytes(int(quant[t][ZZ[k]]) & 255 for k in range(64)))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        sof += bytes([c + 1, (h << 4) | v if c == 0 else 0x11, 0 if c == 0 or len(quant) < 2 else 1])
    out += _seg(0xC2, sof)
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, "big"))
    for i, (comps, ss, se, ah, al) in enumerate(script):
        comps = tuple(comps)
        units = scan_units(width, height, h if ncomp > 1 else 1, v if ncomp > 1 else 1, comps)
        tok = _Tokens()
        _encode_scan(tok, units, coef, ss, se, ah, al, restart, comps)
        if token_hook:
            token_hook(i, tok.intervals)
        freqs = {}
        for iv in tok.intervals:
            for t in iv:
                if t[0] == "s":
                    freqs.setdefault(t[1], {}).setdefault(t[2], 0)
                    freqs[t[1]][t[2]] += 1
        books = {}
        for tab, fr in sorted(freqs.items()):
            counts, symbols = optimal_table(fr)
            books[tab] = code_book(counts, symbols)
            out += _seg(0xC4, bytes([(0 if ss == 0 else 0x10) | tab]) + bytes(counts) + bytes(symbols))
        hdr = bytes([len(comps)])
        for k, c in enumerate(comps):
            hdr += bytes([c + 1, (k << 4) if ss == 0 else 0])
        hdr += bytes([ss, se, (ah << 4) | al])
        data = b""
        for n, iv in enumerate(tok.intervals):
            if n:
                data += bytes([0xFF, 0xD0 + (n - 1) % 8])
            data += _pack(iv, books)
        if raw_scan_hook:
            hdr, data = raw_scan_hook(i, hdr, data)
        out += _seg(0xDA, hdr) + data
    if eoi:
        out += b"\xff\xd9"
    return bytes(out)


# ---------------------------------------------------------------- the model decoder ----
class _Bits:
    def __init__(self, data):
        self.d, self.p, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            self.acc = self.d[self.p] if self.p < len(self.d) else 0
            self.p += 1
            self.n = 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def sym(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise ValueError("bad Huffman code")


def _extend(v, t):
    return v - (1 << t) + 1 if t and v < (1 << (t - 1)) else v


def _intervals(data):
    """a scan's bytes without stuffing, cut at the RSTn markers; ends at any other marker -> (list of bytes, length consumed)"""
    out, cur, p = [], bytearray(), 0
    while p < len(data):
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        nxt = data[p + 1] if p + 1 < len(data) else 0xD9
        if nxt == 0:
            cur.append(0xFF)
            p += 2
        elif 0xD0 <= nxt <= 0xD7:
            out.append(bytes(cur))
            cur = bytearray()
            p += 2
        else:
            break
    out.append(bytes(cur))
    return out, p


def model_decode(data, k_max=63):
    """-> dict(width, height, ncomp, h, v, mcu_cols, mcu_rows, quant[4][64], coef[3], scans=[dict(comps, ss, se, ah, al, max_eobrun, skipped)])"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    p = 2
    quant = np.ones((4, 64), dtype=np.uint16)
    huff, comps, restart, scans, planes = {}, [], 0, [], None
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        p += 2
        if m == 0xD9:
            break
        L = (data[p] << 8) | data[p + 1]
        seg = data[p + 2:p + L]
        p += L
        if m == 0xDB:
            i = 0
            while i < len(seg):
                prec, tid = seg[i] >> 4, seg[i] & 15
                i += 1
                for k in range(64):
                    quant[tid][ZZ[k]] = (seg[i] << 8) | seg[i + 1] if prec else seg[i]
                    i += 2 if prec else 1
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = seg[i + 17 + k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(tc, th)] = table
                i += 17 + n
        elif m == 0xC2:
            height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            for c in range(seg[5]):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                comps.append(dict(id=cid, h=hv >> 4, v=hv & 15, tq=tq))
            if len(comps) == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            h, v = comps[0]["h"], comps[0]["v"]
            mcu_cols, mcu_rows = geometry(width, height, h, v)
            planes = [np.zeros((mcu_cols * mcu_rows * c["h"] * c["v"], 64), dtype=np.int16) for c in comps]
        elif m == 0xDD:
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            sc, tabs = [], []
            for k in range(ns):
                sc.append(next(i for i, x in enumerate(comps) if x["id"] == seg[1 + 2 * k]))
                tabs.append((seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15))
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            ivs, used = _intervals(data[p:])
            p += used
            info = dict(comps=tuple(sc), ss=ss, se=se, ah=ah, al=al, max_eobrun=0, skipped=ss > k_max)
            scans.append(info)
            if info["skipped"]:
                continue
            units = scan_units(width, height, h, v, sc)
            per = restart or len(units)
            for n_iv, first in enumerate(range(0, len(units), per)):
                br = _Bits(ivs[n_iv])
                pred = [0] * ns
                eobrun = 0
                for unit in units[first:first + per]:
                    for c, bi in unit:
                        blk = planes[c][bi]
                        k_sc = sc.index(c)
                        if ss == 0:
                            if ah:
                                if br.bit():
                                    blk[0] |= 1 << al
                            else:
                                t = br.sym(huff[(0, tabs[k_sc][0])])
                                pred[k_sc] += _extend(br.bits(t), t)
                                blk[0] = pred[k_sc] << al
                            continue
                        table = huff[(1, tabs[0][1])]
                        if not ah:
                            if eobrun:
                                eobrun -= 1
                                continue
                            k = ss
                            while k <= se:
                                rs = br.sym(table)
                                r, s = rs >> 4, rs & 15
                                if s:
                                    k += r
                                    blk[ZZ[k]] = _extend(br.bits(s), s) * (1 << al)
                                elif r == 15:
                                    k += 15
                                else:
                                    eobrun = (1 << r) + br.bits(r)
                                    info["max_eobrun"] = max(info["max_eobrun"], eobrun)
                                    eobrun -= 1
                                    break
                                k += 1
                            continue
                        # Figure G.7
                        p1 = 1 << al

                        def correct(z):
                            if br.bit() and not (int(blk[z]) & p1):
                                blk[z] += p1 if blk[z] >= 0 else -p1

                        k = ss
                        if not eobrun:
                            while k <= se:
                                rs = br.sym(table)
                                r, s = rs >> 4, rs & 15
                                val = 0
                                if s:
                                    assert s == 1
                                    val = p1 if br.bit() else -p1
                                elif r != 15:
                                    eobrun = (1 << r) + br.bits(r)
                                    info["max_eobrun"] = max(info["max_eobrun"], eobrun)
                                    break
                                while k <= se:
                                    z = ZZ[k]
                                    if blk[z]:
                                        correct(z)
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if s:
                                    blk[ZZ[k]] = val
                                k += 1
                        if eobrun:
                            while k <= se:
                                if blk[ZZ[k]]:
                                    correct(ZZ[k])
                                k += 1
                            eobrun -= 1
    coef = [np.ascontiguousarray(pl) for pl in planes] + [None] * (3 - len(comps))
    return dict(width=width, height=height, ncomp=len(comps), h=h, v=v, mcu_cols=mcu_cols, mcu_rows=mcu_rows, quant=quant, coef=coef,
                scans=scans)


# ---------------------------------------------------------------- scripts ----
def pil_script(ncomp):
    """the ten-scan script libjpeg's jpeg_simple_progression writes for YCbCr (six scans for grey)"""
    if ncomp == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
            ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def random_coef(rng, width, height, h, v, ncomp=3, density=0.25, amp=40):
    """sparse coefficient planes with every block of the MCU grid filled: [blocks][64] int16 per component"""
    mcu_cols, mcu_rows = geometry(width, height, h if ncomp > 1 else 1, v if ncomp > 1 else 1)
    out = []
    for c in range(ncomp):
        nb = mcu_cols * mcu_rows * (h * v if c == 0 and ncomp > 1 else 1)
        a = rng.integers(-amp, amp + 1, size=(nb, 64)) * (rng.random((nb, 64)) < density)
        a[:, 0] = rng.integers(-500, 500, size=nb)
        out.append(a.astype(np.int16))
    return out


def expected_planes(coef, width, height, h, v, script):
    """What a decoder must deliver for `coef` written under `script`: coefficient k of component c keeps the bits down to the Al of the last
    scan that carried it (DC: arithmetic shift; AC: the magnitude's), and is zero where no scan carried it.  Blocks of the MCU grid outside
    a component's own grid are touched by interleaved scans only."""
    ncomp = len(coef)
    hh, vv = (h, v) if ncomp > 1 else (1, 1)
    mcu_cols, mcu_rows = geometry(width, height, hh, vv)
    out = []
    for c in range(ncomp):
        bw, bh = comp_grid(width, height, hh, vv, c)
        in_grid = np.zeros(len(coef[c]), dtype=bool)
        in_grid[[block_index(mcu_cols, hh, vv, c, bx, by) for by in range(bh) for bx in range(bw)]] = True
        al_grid, al_pad = [None] * 64, [None] * 64
        for comps, ss, se, ah, al in script:
            if c not in comps:
                continue
            for k in range(ss, se + 1):
                al_grid[k] = al
                if len(comps) > 1:
                    al_pad[k] = al
        res = np.zeros_like(coef[c])
        for k in range(64):
            x = coef[c][:, ZZ[k]].astype(np.int64)
            for mask, al in ((in_grid, al_grid[k]), (~in_grid, al_pad[k])):
                if al is None:
                    continue
                val = (x >> al) << al if k == 0 else np.sign(x) * ((np.abs(x) >> al) << al)
                res[mask, ZZ[k]] = val[mask]
        out.append(res)
    return out
