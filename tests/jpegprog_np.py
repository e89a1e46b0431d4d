"""Numpy restatement of the progressive coefficient stage of csrc/jpeg_prog.hip (include/poco_hip.h): the scans of
a progressive JPEG file (poco_amd.jpeg.parse_progressive_jpeg), decoded one after the other as libjpeg's jdphuff.c does, fill the
coefficient buffer that tests/jpegdec_np.py turns into pixels (dequantisation, "islow" inverse DCT, fancy upsampling, colour) - so
the pixels are PIL's, byte for byte, and the device must produce these BYTES.

    decode(data) -> uint8 [H,W,3]                 raises JpegError on a damaged stream
    decode_status(data) -> (pixels | None, status) status as the device's word: 0, ERR_CODE or ERR_SHORT of the first damaged scan
    both take a dict `stats` that receives counters of what the file made the decoder do (longest end-of-band runs, runs of
    exactly 32767, correction bits - also those of blocks wholly inside an end-of-band run of a refinement scan -, symbols and
    how many of them had codes past the lookahead table, the levels of the scan order, DC scans of one component)

The bit reader is the device's: bits MSB first from the scan's bytes with the 0x00 behind every 0xFF skipped; a scan that asks
for more bits than it has is ERR_SHORT.  Damage ends the scan: a window that holds no code, a run that passes Se, an end-of-band
run that passes the scan's last block, a refinement symbol whose size is neither 0 nor 1 (all ERR_CODE)."""
from __future__ import annotations

import numpy as np

from tests import jpegdec_np as J
from poco_amd.jpeg import _ZIGZAG, parse_progressive_jpeg

ERR_CODE, ERR_SHORT = 1, 2
ZZ = _ZIGZAG.tolist()


class JpegError(J.JpegError):
    def __init__(self, msg, status=ERR_CODE):
        super().__init__(msg)
        self.status = status


class Bits:
    """The scan's bits, MSB first."""

    def __init__(self, data: bytes, lo: int, hi: int, stats=None):
        self.stats = stats
        raw = data[lo:hi].replace(b"\xff\x00", b"\xff")
        self.real = 8 * len(raw)
        self.total = self.real + 64                        # zeros behind the end, so that a 16-bit window can always be read
        self.val = int.from_bytes(raw + bytes(8), "big")
        self.pos = 0

    def peek16(self) -> int:
        if self.pos >= self.real:
            raise JpegError("the scan's bytes end before its blocks do", ERR_SHORT)
        return (self.val >> (self.total - self.pos - 16)) & 0xFFFF

    def skip(self, n: int) -> None:
        self.pos += n
        if self.pos > self.real:
            raise JpegError("the scan's bytes end before its blocks do", ERR_SHORT)

    def get(self, n: int) -> int:
        if n == 0:
            return 0
        if self.pos + n > self.real:
            raise JpegError("the scan's bytes end before its blocks do", ERR_SHORT)
        v = (self.val >> (self.total - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        return v

    def symbol(self, tab: J.HuffTable) -> int:
        ln, sym = tab.lookup(self.peek16())
        if ln == 0:
            raise JpegError("no Huffman code at bit %d" % self.pos)
        self.skip(ln)
        if self.stats is not None:
            self.stats["symbols"] += 1
            self.stats["long_codes"] += ln > J.LOOKAHEAD   # the device's slow path: no entry in the lookahead table
        return sym

    def value(self, s: int) -> int:
        """T.81 F.2.2.1 EXTEND of the next s bits."""
        if s == 0:
            return 0
        v = self.get(s)
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


class Geometry:
    def __init__(self, info):
        self.hs, self.vs, self.ncomp = info.hsamp, info.vsamp, info.ncomp
        self.mcuy, self.mcux = info.mcus
        self.bpm = 1 if info.ncomp == 1 else info.hsamp * info.vsamp + 2
        self.nblocks = self.mcuy * self.mcux * self.bpm
        # the components' own sizes in blocks: what a scan of one component covers
        self.bw = [-(-info.width // 8)] + [-(-(-(-info.width // info.hsamp)) // 8)] * (info.ncomp - 1)
        self.bh = [-(-info.height // 8)] + [-(-(-(-info.height // info.vsamp)) // 8)] * (info.ncomp - 1)

    def block(self, c: int, bx: int, by: int) -> int:
        """Index into the MCU-ordered coefficient buffer of block (bx, by) of component c."""
        if c == 0:
            return ((by // self.vs) * self.mcux + bx // self.hs) * self.bpm + (by % self.vs) * self.hs + bx % self.hs
        return (by * self.mcux + bx) * self.bpm + self.hs * self.vs + c - 1

    def scan_blocks(self, comps):
        """[(component index within the scan, block)] in the scan's order."""
        if len(comps) == 1:
            c = comps[0]
            return [(0, self.block(c, bx, by)) for by in range(self.bh[c]) for bx in range(self.bw[c])]
        comp_of = [0] * (self.hs * self.vs) + list(range(1, self.ncomp))
        return [(comp_of[k], m * self.bpm + k) for m in range(self.mcuy * self.mcux) for k in range(self.bpm)]


def dc_first(bits, scan, blocks, coef, tabs):
    pred = [0] * len(scan.comps)
    for k, blk in blocks:
        s = bits.symbol(tabs[k])
        pred[k] += bits.value(s)
        coef[blk, 0] = pred[k] << scan.al


def dc_refine(bits, scan, blocks, coef):
    for _, blk in blocks:
        if bits.get(1):
            coef[blk, 0] |= 1 << scan.al


def ac_first(bits, scan, blocks, coef, tab, stats):
    i, n = 0, len(blocks)
    while i < n:
        blk = blocks[i][1]
        k = scan.ss
        while k <= scan.se:
            sym = bits.symbol(tab)
            r, s = sym >> 4, sym & 15
            if s:
                k += r
                if k > scan.se:
                    raise JpegError("a run passes Se")
                coef[blk, ZZ[k]] = bits.value(s) << scan.al
            elif r == 15:
                k += 15
            else:
                run = (1 << r) + bits.get(r) - 1          # blocks after this one that are at their end of band too
                if run > n - 1 - i:
                    raise JpegError("an end-of-band run passes the last block")
                stats["eobrun"] = max(stats["eobrun"], run + 1)
                stats["eobrun_cap"] += run + 1 == 0x7FFF
                i += run
                break
            k += 1
        i += 1


def _correct(bits, coef, blk, k, p1):
    """A correction bit for the non-zero coefficient at zigzag index k."""
    v = int(coef[blk, ZZ[k]])
    if bits.get(1) and (v & p1) == 0:
        coef[blk, ZZ[k]] = v + p1 if v >= 0 else v - p1


def ac_refine(bits, scan, blocks, coef, tab, stats):
    p1 = 1 << scan.al
    eobrun = 0
    for i, (_, blk) in enumerate(blocks):
        k = scan.ss
        inside = eobrun > 0                                # the whole block lies inside an end-of-band run
        if eobrun == 0:
            while k <= scan.se:
                sym = bits.symbol(tab)
                r, s = sym >> 4, sym & 15
                new = 0
                if s:
                    if s != 1:
                        raise JpegError("a refinement symbol of size %d" % s)
                    new = p1 if bits.get(1) else -p1
                elif r != 15:
                    eobrun = (1 << r) + bits.get(r)
                    if eobrun - 1 > len(blocks) - 1 - i:
                        raise JpegError("an end-of-band run passes the last block")
                    stats["refine_eobrun"] = max(stats["refine_eobrun"], eobrun)
                    break
                else:
                    stats["refine_zrl"] += 1
                while k <= scan.se:                        # r zeros are skipped, every non-zero on the way takes a correction bit
                    if coef[blk, ZZ[k]] != 0:
                        _correct(bits, coef, blk, k, p1)
                        stats["corrections"] += 1
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if new:
                    if k > scan.se:
                        raise JpegError("a run passes Se")
                    coef[blk, ZZ[k]] = new
                k += 1
        if eobrun > 0:
            while k <= scan.se:
                if coef[blk, ZZ[k]] != 0:
                    _correct(bits, coef, blk, k, p1)
                    stats["corrections"] += 1
                    stats["eob_corrections"] += inside
                k += 1
            eobrun -= 1


def coefficients(info, stats=None):
    """(int32 [MCUs * blocks per MCU, 64] quantised coefficients in natural order, status): the scans in file order; the first
    damaged scan ends the decode."""
    g = Geometry(info)
    coef = np.zeros((g.nblocks, 64), np.int32)
    stats = stats if stats is not None else {}
    for key in ("eobrun", "eobrun_cap", "refine_eobrun", "refine_zrl", "corrections", "eob_corrections", "symbols", "long_codes",
                "levels", "dc_alone", "dc_refine_ragged_luma"):
        stats.setdefault(key, 0)
    depth = np.zeros((info.ncomp, 64), np.int64)           # scans that have touched each (component, coefficient) so far
    for scan in info.scans:
        bits = Bits(info.data, scan.offset, scan.offset + scan.length, stats)
        blocks = g.scan_blocks(scan.comps)
        band = depth[list(scan.comps), scan.ss:scan.se + 1]
        depth[list(scan.comps), scan.ss:scan.se + 1] = band.max() + 1      # the device's level of this scan, plus one
        stats["levels"] = max(stats["levels"], int(depth.max()))
        if scan.ss == 0 and len(scan.comps) == 1 and info.ncomp > 1:
            stats["dc_alone"] += 1
            # luma's own raster is narrower than the MCU raster: the walk differs from the interleaved one
            stats["dc_refine_ragged_luma"] += scan.ah > 0 and scan.comps[0] == 0 and g.bw[0] % g.hs != 0
        try:
            if scan.ss == 0 and scan.ah == 0:
                dc_first(bits, scan, blocks, coef, [J.HuffTable(*t) for t in scan.dc])
            elif scan.ss == 0:
                dc_refine(bits, scan, blocks, coef)
            elif scan.ah == 0:
                ac_first(bits, scan, blocks, coef, J.HuffTable(*scan.ac), stats)
            else:
                ac_refine(bits, scan, blocks, coef, J.HuffTable(*scan.ac), stats)
        except JpegError as e:
            return coef, e.status
    return coef, 0


def pixels(info, coef) -> np.ndarray:
    """tests/jpegdec_np.py's way from coefficients to the picture."""
    pl = J.planes(info, coef)
    H, W = info.height, info.width
    if info.ncomp == 1:
        y = pl[0][:H, :W]
        return np.stack([y, y, y], -1).astype(np.uint8)
    cw, ch = -(-W // info.hsamp), -(-H // info.vsamp)
    chroma = []
    for p in pl[1:]:
        p = p[:ch, :cw]
        if info.hsamp == 2 and cw > 2:
            p = J.upsample_h2v2(p) if info.vsamp == 2 else J.upsample_h2v1(p)
        else:
            p = np.repeat(np.repeat(p, info.vsamp, 0), info.hsamp, 1)
        chroma.append(p[:H, :W])
    return J.ycc_to_rgb(pl[0][:H, :W], chroma[0], chroma[1])


def decode_status(data: bytes, stats=None):
    info = parse_progressive_jpeg(data)
    if info is None:
        raise JpegError("not a progressive JPEG this decoder takes")
    coef, status = coefficients(info, stats)
    if status == 0 and info.cut:
        # a file cut short whose script ends above Al = 0 is damaged even when the cut falls exactly between two scans
        final = np.zeros((info.ncomp, 64), np.int64)
        for sc in info.scans:
            final[list(sc.comps), sc.ss:sc.se + 1] = sc.al
        if final.any():
            status = ERR_SHORT
    return (pixels(info, coef) if status == 0 else None), status


def decode(data: bytes) -> np.ndarray:
    px, status = decode_status(data)
    if status:
        raise JpegError("damaged stream", status)
    return px
