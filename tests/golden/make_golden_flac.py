#!/usr/bin/env python
"""tests/golden/jfk_head.flac: the first FRAMES frames of the reference's tests/jfk.flac (24-bit stereo 44.1 kHz, LPC +
Rice coded, fixed 4608-sample blocks), byte for byte, behind its own metadata blocks.  Only STREAMINFO changes: the total
sample count and the MD5 signature, which becomes the MD5 of the prefix of the whole file's decoded PCM.  That decode is
itself checked against the encoder's MD5 signature of the whole stream, so the fixture stays self-validating.  Prints the
SHA-256 of the kept PCM and its sample count, which tests/test_audio_io.py pins.

    python tests/golden/make_golden_flac.py <path of the reference's tests/jfk.flac>
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from whisper_amd.audio import decode_flac  # noqa: E402  (verifies frame CRCs and the STREAMINFO MD5)

FRAMES = 16
OUT = os.path.join(HERE, "jfk_head.flac")


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def frame_offset(data: bytes, start: int, number: int) -> int:
    """byte offset of the frame header with this frame number (fixed-blocksize stream; sync code + header CRC-8 checked)"""
    p = start
    while True:
        p = data.index(b"\xff\xf8", p)
        b = data[p + 4]                                   # first byte of the UTF-8 coded frame number
        n_extra = 0 if b < 0x80 else (1 if b >> 5 == 6 else 2 if b >> 4 == 14 else 3 if b >> 3 == 30 else -1)
        if n_extra >= 0:
            v = b if n_extra == 0 else b & (0x3F >> n_extra)
            for i in range(n_extra):
                v = (v << 6) | (data[p + 5 + i] & 0x3F)
            end = p + 5 + n_extra
            bs_code, rate_code = data[p + 2] >> 4, data[p + 2] & 15
            end += {6: 1, 7: 2}.get(bs_code, 0) + {12: 1, 13: 2, 14: 2}.get(rate_code, 0)
            if v == number and crc8(data[p:end]) == data[end]:
                return p
        p += 1


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    data = open(sys.argv[1], "rb").read()
    pcm, rate, bps = decode_flac(data)                    # the whole stream, MD5-verified
    p, audio_start = 4, None
    while audio_start is None:
        last, length = data[p] >> 7, int.from_bytes(data[p + 1: p + 4], "big")
        if data[p] & 0x7F == 0:
            si = p + 4
            block = int.from_bytes(data[si + 2: si + 4], "big")
        p += 4 + length
        if last:
            audio_start = p
    cut = frame_offset(data, audio_start, FRAMES)
    n = FRAMES * block
    kept = pcm[:n]
    # PCM as the encoder's MD5 covers it: interleaved little-endian samples of bps / 8 bytes each
    raw = b"".join(int(v).to_bytes(bps // 8, "little", signed=True) for v in kept.reshape(-1))
    x = int.from_bytes(data[si + 10: si + 18], "big")
    x = (x >> 36 << 36) | n
    head = bytearray(data[:audio_start])
    head[si + 10: si + 18] = x.to_bytes(8, "big")
    head[si + 18: si + 34] = hashlib.md5(raw).digest()
    out = bytes(head) + data[audio_start:cut]
    again, rate2, bps2 = decode_flac(out)
    assert (rate2, bps2) == (rate, bps) and (again == kept).all()
    with open(OUT, "wb") as f:
        f.write(out)
    print(f"{OUT}: {len(out)} bytes, {n} samples x {pcm.shape[1]} channels, "
          f"PCM sha256 {hashlib.sha256(kept.astype('<i4').tobytes()).hexdigest()}")


if __name__ == "__main__":
    main()
