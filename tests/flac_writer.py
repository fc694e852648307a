"""A test-side FLAC encoder (RFC 9639) that can say everything the decoders have to read — not a good encoder, a complete
one.  Per subframe: CONSTANT, VERBATIM, FIXED 0 - 4, LPC of order 1 - 32 with a chosen precision, shift and any integer
coefficients (the residual is whatever they leave); Rice partition orders with a per-partition parameter, 4- or 5-bit
parameters (Rice2), escaped partitions with raw n-bit residuals (n = 0 included); wasted bits.  Per frame: channel
assignments 0 - 10, any block size, fixed or variable blocking with the coded number in all its UTF-8-style lengths.  Per
stream: 8 / 12 / 16 / 20 / 24 (or any 4 - 32) bits, 1 - 8 channels, a short last frame, an ID3v2 prefix, trailing bytes, the
STREAMINFO MD5.

`matrix()` is the set of streams the FLAC tests share (CPU: tests/test_flac_frames_cpu.py, GPU: tests/test_flac_device_gpu.py),
`planted(n)` a stream whose payload holds n complete, valid frame headers, `rejections()` the tampered streams."""
import hashlib
from functools import lru_cache

import numpy as np


# ------------------------------------------------------------------------------------------------ bits and CRCs
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, bits: int):
        if bits == 0:
            return
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc = (self.acc << bits) | value
        self.n += bits
        if self.n >= 256:
            self._flush()

    def put_signed(self, value: int, bits: int):
        assert -(1 << (bits - 1)) <= value < (1 << (bits - 1)), (value, bits)
        self.put(value & ((1 << bits) - 1), bits)

    def unary(self, q: int):
        self.put(1, q + 1)

    def _flush(self):
        k = self.n // 8
        rest = self.n - 8 * k
        self.out += (self.acc >> rest).to_bytes(k, "big")
        self.acc &= (1 << rest) - 1
        self.n = rest

    def align(self):
        if self.n % 8:
            self.put(0, 8 - self.n % 8)

    def bytes(self) -> bytes:
        self.align()
        self._flush()
        return bytes(self.out)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def coded_number(v: int) -> bytes:
    """the UTF-8-style number of a frame header: 1 byte below 2^7, then 2 .. 7 bytes for up to 11, 16, 21, 26, 31, 36 bits"""
    if v < 0x80:
        return bytes([v])
    for n, bits in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if v < (1 << bits):
            lead = (0xFF << (8 - n)) & 0xFF
            out = [lead | (v >> (6 * (n - 1)))]
            out += [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(n - 2, -1, -1)]
            return bytes(out)
    raise ValueError(v)


# ------------------------------------------------------------------------------------------------ subframes
class Sub:
    """how one subframe is coded.  kind: "constant" | "verbatim" | "fixed" | "lpc"; order; for lpc: precision (1 - 15), shift
    (0 - 15), coefs (order integers); residual: porder (partitions = 2^porder), rice2 (5-bit parameters), ks = one entry per
    partition: a Rice parameter, None (chosen from the residual) or ("esc", n) for raw n-bit residuals (n None: as few bits
    as hold them, 0 if all are zero); wasted: low zero bits the samples are known to have (they must)."""

    def __init__(self, kind="verbatim", order=0, precision=12, shift=10, coefs=None, porder=0, rice2=False, ks=None, wasted=0):
        self.kind, self.order, self.precision, self.shift = kind, order, precision, shift
        self.coefs, self.porder, self.rice2, self.ks, self.wasted = coefs, porder, rice2, ks, wasted


_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def _residual(w: Bits, res, blocksize: int, order: int, sub: Sub):
    w.put(1 if sub.rice2 else 0, 2)
    pbits, esc = (5, 31) if sub.rice2 else (4, 15)
    porder = sub.porder
    assert blocksize % (1 << porder) == 0 and (blocksize >> porder) >= order, (blocksize, porder, order)
    w.put(porder, 4)
    at = 0
    for part in range(1 << porder):
        count = (blocksize >> porder) - (order if part == 0 else 0)
        rs = res[at: at + count]
        at += count
        k = sub.ks[part] if sub.ks is not None else None
        if isinstance(k, tuple):
            n = k[1]
            if n is None:
                n = 0 if not any(rs) else max(max(r.bit_length() if r >= 0 else (~r).bit_length() for r in rs) + 1, 1)
            w.put(esc, pbits)
            w.put(n, 5)
            for r in rs:
                if n:
                    w.put_signed(r, n)
                else:
                    assert r == 0
            continue
        if k is None:
            mean = sum(abs(r) for r in rs) // max(1, len(rs))
            k = min(mean.bit_length(), esc - 1)
        assert 0 <= k < esc
        w.put(k, pbits)
        for r in rs:
            u = 2 * r if r >= 0 else -2 * r - 1
            w.unary(u >> k)
            w.put(u & ((1 << k) - 1), k)
    assert at == len(res)


def _subframe(w: Bits, x, bps: int, sub: Sub):
    """x: python ints of one channel of one block, `bps` bits wide"""
    n = len(x)
    wasted = sub.wasted
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in x)
        x = [v >> wasted for v in x]
        bps -= wasted
    code = {"constant": 0, "verbatim": 1}.get(sub.kind)
    if sub.kind == "fixed":
        code = 8 + sub.order
    elif sub.kind == "lpc":
        code = 32 + sub.order - 1
    w.put(0, 1)
    w.put(code, 6)
    if wasted:
        w.put(1, 1)
        w.unary(wasted - 1)
    else:
        w.put(0, 1)
    if sub.kind == "constant":
        assert all(v == x[0] for v in x)
        w.put_signed(x[0], bps)
    elif sub.kind == "verbatim":
        for v in x:
            w.put_signed(v, bps)
    else:
        order = sub.order
        coefs, shift = (_FIXED[order], 0) if sub.kind == "fixed" else (tuple(sub.coefs), sub.shift)
        assert len(coefs) == order <= n
        for v in x[:order]:
            w.put_signed(v, bps)
        if sub.kind == "lpc":
            w.put(sub.precision - 1, 4)
            w.put_signed(shift, 5)
            for c in coefs:
                w.put_signed(c, sub.precision)
        res = [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, n)]
        _residual(w, res, n, order, sub)


# ------------------------------------------------------------------------------------------------ frames and streams
_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def frame_header(blocksize: int, rate: int, channels_code: int, bps: int, number: int, variable: bool) -> bytes:
    w = Bits()
    w.put(0xFFF8 | int(variable), 16)
    bs_code = _BS_CODES.get(blocksize, 6 if blocksize <= 256 else 7)
    w.put(bs_code, 4)
    w.put(_SR_CODES.get(rate, 0), 4)
    w.put(channels_code, 4)
    w.put(_SS_CODES.get(bps, 0), 3)
    w.put(0, 1)
    for b in coded_number(number):
        w.put(b, 8)
    if bs_code == 6:
        w.put(blocksize - 1, 8)
    elif bs_code == 7:
        w.put(blocksize - 1, 16)
    head = w.bytes()
    return head + bytes([crc8(head)])


def encode_frame(block, rate: int, bps: int, number: int, variable: bool, assignment: int, subs) -> bytes:
    """block: [blocksize][channels] ints; assignment: 0 - 7 independent (must be channels - 1), 8 left/side, 9 side/right,
    10 mid/side (stereo); subs: one Sub per channel"""
    cols = [[int(v) for v in block[:, c]] for c in range(block.shape[1])]
    widths = [bps] * len(cols)
    if assignment >= 8:
        left, right = cols
        side = [a - b for a, b in zip(left, right)]
        if assignment == 8:
            cols, widths = [left, side], [bps, bps + 1]
        elif assignment == 9:
            cols, widths = [side, right], [bps + 1, bps]
        else:
            cols, widths = [[(a + b) >> 1 for a, b in zip(left, right)], side], [bps, bps + 1]
    else:
        assert assignment == len(cols) - 1
    w = Bits()
    for b in frame_header(len(block), rate, assignment, bps, number, variable):
        w.put(b, 8)
    for x, width, sub in zip(cols, widths, subs):
        _subframe(w, x, width, sub)
    body = w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def pcm_md5(pcm, bps: int) -> bytes:
    nb = (bps + 7) // 8
    raw = np.ascontiguousarray(pcm, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :nb]
    return hashlib.md5(raw.tobytes()).digest()


def streaminfo(min_block, max_block, rate, channels, bps, total, md5) -> bytes:
    w = Bits()
    w.put(min_block, 16); w.put(max_block, 16); w.put(0, 24); w.put(0, 24)
    w.put(rate, 20); w.put(channels - 1, 3); w.put(bps - 1, 5); w.put(total, 36)
    return w.bytes() + md5


def id3v2(payload: int) -> bytes:
    size = bytes([(payload >> 21) & 127, (payload >> 14) & 127, (payload >> 7) & 127, payload & 127])
    return b"ID3\x04\x00\x00" + size + bytes((i * 37 + 11) & 0x7F for i in range(payload))


def encode_stream(pcm, rate: int, bps: int, blocksizes, *, subs=None, assignment=None, variable=False, numbers=None,
                  first_number=0, id3=0, trailing=b"", total=None, md5=True, padding=0):
    """pcm [n][channels] -> (stream bytes, frame offsets).  blocksizes: an int (the last block is what is left) or the list of
    block sizes; subs(frame, channel, blocksize) -> Sub (default verbatim); assignment(frame) -> 0 - 10 (default independent); numbers:
    the coded number of every frame (default: frame number from first_number, or the sample number of a variable stream);
    total / md5: what STREAMINFO says (default: the truth)."""
    pcm = np.asarray(pcm)
    n, channels = pcm.shape
    if isinstance(blocksizes, int):
        blocksizes = [min(blocksizes, n - at) for at in range(0, n, blocksizes)]
    assert sum(blocksizes) == n
    frames, at = [], 0
    for f, bs in enumerate(blocksizes):
        number = numbers[f] if numbers is not None else (first_number + at if variable else first_number + f)
        a = assignment(f) if assignment is not None else channels - 1
        ss = [subs(f, c, bs) if subs is not None else Sub() for c in range(channels)]
        frames.append(encode_frame(pcm[at: at + bs], rate, bps, number, variable, a, ss))
        at += bs
    digest = pcm_md5(pcm, bps) if md5 is True else (md5 or bytes(16))
    info = streaminfo(min(blocksizes), max(max(blocksizes), 16), rate, channels, bps, n if total is None else total, digest)
    head = (id3v2(id3) if id3 else b"") + b"fLaC"
    if padding:
        head += bytes([0]) + len(info).to_bytes(3, "big") + info + bytes([0x81]) + padding.to_bytes(3, "big") + bytes(padding)
    else:
        head += bytes([0x80]) + len(info).to_bytes(3, "big") + info
    offsets, pos = [], len(head)
    for fr in frames:
        offsets.append(pos)
        pos += len(fr)
    return head + b"".join(frames) + trailing, offsets


# ------------------------------------------------------------------------------------------------ the shared cases
def signal(n: int, channels: int, bps: int, seed: int) -> np.ndarray:
    """tones plus noise at about a quarter of full scale, correlated between the channels, int32 [n][channels]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    f = 0.01 + 0.02 * np.arange(channels)[None, :]
    x = 0.2 * np.sin(2 * np.pi * 0.013 * t) + 0.05 * np.sin(2 * np.pi * f * t) + 0.004 * rng.standard_normal((n, channels))
    return np.round(x * (1 << (bps - 1))).astype(np.int64).clip(-(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int32)


def _lpc(order: int, precision: int, shift: int, seed: int) -> Sub:
    """a decaying predictor 2 x[-1] - x[-2] flavoured with small random taps: integer coefficients that fit `precision`"""
    rng = np.random.default_rng(seed)
    a = np.zeros(order)
    a[0] = 0.9 if order == 1 else 1.6
    if order > 1:
        a[1] = -0.7
    a[2:] = rng.uniform(-0.02, 0.02, max(0, order - 2))
    lim = (1 << (precision - 1)) - 1
    coefs = [int(v) for v in np.clip(np.round(a * (1 << shift)), -lim - 1, lim)]
    return Sub("lpc", order, precision, shift, coefs)


def varied(seed: int = 0):
    """subs(frame, channel, blocksize): cycles through the subframe kinds, predictor orders, partition orders and residual
    codings that the block size allows, so that a stream of a few dozen frames holds all of them"""
    def subs(f: int, c: int, blocksize: int) -> Sub:
        pmax = 0
        while pmax < 4 and blocksize % (2 << pmax) == 0 and (blocksize >> (pmax + 1)) >= 4:
            pmax += 1
        i = f * 3 + c * 5 + seed
        kind = i % 9
        porder = (i // 2) % (pmax + 1)
        room = blocksize >> porder                    # the first partition must hold the warm-up samples
        if kind == 0:
            return Sub("verbatim")
        if kind <= 4:
            s = Sub("fixed", min(kind if kind < 4 else (i // 9) % 5, room, blocksize), porder=porder)
        else:
            order = min((1, 2, 8, 12, 32)[(i // 9) % 5], room, blocksize, 32)
            s = _lpc(order, (12, 15, 7, 10)[i % 4], (10, 13, 5, 8)[i % 4], i)
            s.porder = porder
        s.rice2 = (i % 5) == 3
        if (i % 7) == 2:                              # one escaped partition among the Rice ones
            s.ks = [("esc", None) if p == (i % (1 << porder)) else None for p in range(1 << porder)]
        return s
    return subs


@lru_cache(maxsize=None)
def matrix():
    """[(name, stream bytes, pcm int32 [n][channels], rate, bps)] — built once per process"""
    cases = []

    def add(name, pcm, rate, bps, blocksizes, **kw):
        data, _ = encode_stream(pcm, rate, bps, blocksizes, **kw)
        cases.append((name, data, np.ascontiguousarray(pcm, dtype=np.int32), rate, bps))

    # block size x frame count x channels: a full wave of frames, a wave plus one, more than two waves; one huge frame
    for bs, frames, ch, bps in ((16, 130, 2, 16), (192, 65, 1, 16), (256, 130, 3, 16), (256, 63, 2, 24), (256, 64, 8, 16),
                                (1000, 5, 2, 20), (4096, 1, 2, 16), (4096, 9, 2, 24), (65535, 1, 1, 16)):
        pcm = signal(bs * frames, ch, bps, seed=bs + frames)
        add(f"bs{bs}_f{frames}_ch{ch}_b{bps}", pcm, 44100, bps, bs, subs=varied(seed=ch),
            assignment=(lambda f: 8 + f % 3) if ch == 2 else None)
    # sample sizes and channel counts, independent channels
    for bps in (8, 12, 16, 20, 24):
        for ch in (1, 4, 5, 6, 7):
            if (bps, ch) in ((8, 1), (12, 4), (16, 5), (20, 6), (24, 7), (16, 1)):
                add(f"b{bps}_ch{ch}", signal(1500, ch, bps, seed=bps * ch), 48000 if bps != 12 else 12345, bps, 512,
                    subs=varied(seed=bps))
    # every stereo assignment with every subframe family, a short last frame
    for a in (1, 8, 9, 10):
        add(f"assign{a}_short_last", signal(2000, 2, 16, seed=a), 16000, 16, 576, subs=varied(seed=a), assignment=lambda f, a=a: a)
    # constant subframes, wasted bits, escapes with n = 0, explicit per-partition parameters, Rice2 with a large parameter
    x = signal(1024, 2, 16, seed=5)
    x[:, 0] = -1234
    x[:, 1] = (x[:, 1] >> 3) << 3
    add("constant_and_wasted", x, 22050, 16, 256,
        subs=lambda f, c, n: Sub("constant") if c == 0 else Sub("fixed", 2, porder=2, ks=[3, 4, None, 5], wasted=3))
    z = np.zeros((512, 1), np.int32)
    z[256:, 0] = signal(256, 1, 24, seed=6)[:, 0]
    add("escape_zero_bits", z, 8000, 24, 256,
        subs=lambda f, c, n: Sub("fixed", 0, porder=1, ks=[("esc", 0), ("esc", 0)]) if f == 0 else
        Sub("fixed", 1, porder=1, rice2=True, ks=[20, ("esc", 25)]))
    # variable block size: sample numbers of 1 .. 7 coded bytes; fixed block size: frame numbers beyond one byte
    sizes = [16, 100, 256, 1000, 17, 4096, 300]
    add("variable_numbers", signal(sum(sizes), 2, 16, seed=7), 44100, 16, sizes, variable=True, subs=varied(seed=2),
        numbers=[0, 200, 5000, 100000, 3000000, 100000000, 30000000000])
    add("frame_numbers_multibyte", signal(64 * 40, 1, 16, seed=8), 44100, 16, 64, first_number=100, subs=varied())
    # container: ID3v2 prefix, a PADDING block, trailing bytes (an ID3v1-sized tag)
    add("id3_padding_trailing", signal(3000, 2, 16, seed=9), 44100, 16, 1152, subs=varied(), id3=77, padding=40,
        trailing=b"TAG" + bytes(125))
    return cases


def plant_payload(n_plants: int, length: int, rate: int = 44100) -> np.ndarray:
    """int8 samples of a mono 8-bit stream whose bytes hold `n_plants` complete frame headers (CRC-8 correct, codes
    consistent with a mono 8-bit stream, block size 256) between bytes that cannot start one"""
    fake = frame_header(256, rate, 0, 8, 5, False)
    raw = bytearray((i * 29 + 3) % 0x7F for i in range(length))           # no 0xFF anywhere else
    gap = length // (n_plants + 1)
    for k in range(n_plants):
        at = (k + 1) * gap
        if at % 1024 > 1024 - 8:                                          # keep a plant inside one block of 1024
            at -= 8
        raw[at: at + len(fake)] = fake
    return np.frombuffer(bytes(raw), np.int8).astype(np.int32)[:, None]


@lru_cache(maxsize=None)
def planted(n_plants: int):
    """(stream, pcm, rate, bps): verbatim 8-bit mono — byte-aligned subframes, so the samples are the stream's bytes"""
    pcm = plant_payload(n_plants, 4096)
    data, offsets = encode_stream(pcm, 44100, 8, 1024)
    fake = frame_header(256, 44100, 0, 8, 5, False)
    assert data.count(fake) == n_plants, "a plant straddles a subframe boundary"
    return data, np.ascontiguousarray(pcm, dtype=np.int32), 44100, 8


@lru_cache(maxsize=None)
def rejections():
    """{name: stream} — each fails the frame checks (and wh_flac_decode) in its own way; "md5" fails the MD5 only"""
    pcm = signal(256 * 6, 2, 16, seed=11)
    good, offsets = encode_stream(pcm, 44100, 16, 256, subs=varied())
    out = {}
    b = bytearray(good); b[offsets[2] + 20] ^= 0x10; out["payload_byte"] = bytes(b)
    b = bytearray(good); b[offsets[3] + 2] ^= 0x01; out["header_byte"] = bytes(b)
    out["cut_mid_frame"] = good[: offsets[5] + 30]
    out["chain_gap"] = good[: offsets[2]] + good[offsets[3]:]
    out["total_too_large"] = encode_stream(pcm, 44100, 16, 256, subs=varied(), total=len(pcm) + 1)[0]
    out["md5"] = encode_stream(pcm, 44100, 16, 256, subs=varied(), md5=bytes(range(1, 17)))[0]
    return out, good, pcm


# ------------------------------------------------------------------------------------------------ long streams, quickly
def _crc16_many(frames) -> list:
    """crc16 of every byte string of `frames`, all at once: the loop runs over the byte index, numpy over the frames"""
    table = np.array(_CRC16, dtype=np.uint16)
    out = []
    for lo in range(0, len(frames), 1024):
        part = frames[lo: lo + 1024]
        lens = np.array([len(f) for f in part])
        buf = np.zeros((len(part), int(lens.max())), dtype=np.uint8)
        for i, f in enumerate(part):
            buf[i, : len(f)] = np.frombuffer(f, np.uint8)
        c = np.zeros(len(part), dtype=np.uint16)
        for col in range(buf.shape[1]):
            nxt = ((c << 8) & 0xFFFF) ^ table[(c >> 8) ^ buf[:, col]]
            c = np.where(col < lens, nxt, c).astype(np.uint16)
        out += [int(v) for v in c]
    return out


def _bits_of(value: int, bits: int) -> np.ndarray:
    return np.array([(value >> (bits - 1 - i)) & 1 for i in range(bits)], dtype=np.uint8)


def _fast_subframe(x: np.ndarray, bps: int) -> np.ndarray:
    """FIXED order 2, one Rice partition (Rice2 when the parameter needs it) -> the subframe's bits, one per uint8"""
    x = x.astype(np.int64)
    res = x[2:] - 2 * x[1:-1] + x[:-2]
    u = np.where(res >= 0, 2 * res, -2 * res - 1)
    k = int(max(0, int(np.mean(u)) + 1).bit_length() - 1)
    head = [_bits_of(0b0001010, 7), _bits_of(0, 1), _bits_of(int(x[0]) & ((1 << bps) - 1), bps), _bits_of(int(x[1]) & ((1 << bps) - 1), bps)]
    head += [_bits_of(0, 2), _bits_of(0, 4), _bits_of(k, 4)] if k < 15 else [_bits_of(1, 2), _bits_of(0, 4), _bits_of(k, 5)]
    q = u >> k
    ends = np.cumsum(q + 1 + k)
    one = ends - k - 1                                    # the stop bit of every code
    bits = np.zeros(int(ends[-1]) if len(ends) else 0, dtype=np.uint8)
    bits[one] = 1
    if k:
        shifts = np.arange(k - 1, -1, -1)
        bits[(one[:, None] + 1 + np.arange(k)[None, :]).ravel()] = ((u[:, None] >> shifts[None, :]) & 1).astype(np.uint8).ravel()
    return np.concatenate(head + [bits])


def encode_stream_fast(pcm, rate: int, bps: int, blocksize: int = 4096) -> bytes:
    """a long stream in seconds instead of hours: independent channels, FIXED order 2 subframes with one Rice partition each
    (what a real encoder's fastest setting does), vectorised over the samples of a subframe; MD5 and CRCs as always"""
    pcm = np.asarray(pcm)
    n, channels = pcm.shape
    assert blocksize >= 16 and channels <= 8
    bodies = []
    for f, at in enumerate(range(0, n, blocksize)):
        block = pcm[at: at + blocksize]
        head = frame_header(len(block), rate, channels - 1, bps, f, False)
        if len(block) < 3:
            w = Bits()
            for c in range(channels):
                _subframe(w, [int(v) for v in block[:, c]], bps, Sub())
            bodies.append(head + w.bytes())
            continue
        bits = np.concatenate([_fast_subframe(block[:, c], bps) for c in range(channels)])
        bodies.append(head + np.packbits(bits).tobytes())
    frames = [b + c.to_bytes(2, "big") for b, c in zip(bodies, _crc16_many(bodies))]
    blocks = [min(blocksize, n - at) for at in range(0, n, blocksize)]
    info = streaminfo(min(blocks), max(max(blocks), 16), rate, channels, bps, n, pcm_md5(pcm, bps))
    return b"fLaC" + bytes([0x80]) + len(info).to_bytes(3, "big") + info + b"".join(frames)
