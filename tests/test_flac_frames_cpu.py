"""The frame-parallel FLAC decode without a GPU: wh_flac_decode_frames (csrc/flac_decode.c) runs the algorithm of
csrc/flac.hip — scan every offset for a frame header, decode every candidate on its own, chain, compact — serially, from the
same per-frame core (csrc/flac_core.h).  Held against the sequential decoder wh_flac_decode, bit for bit, on the streams of
tests/flac_writer.py; false frame headers planted in the payload; tampered streams; the routing of the Python options."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import flac_writer as fw
import whisper_amd
from whisper_amd import audio as A
from whisper_amd import hip

import os
JFK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jfk_head.flac")
FLAC_E_UNSUP, FLAC_E_REJECT = -5, -10


def decode_frames(data: bytes, cand_cap: int = 4096):
    """wh_flac_decode_frames -> (rc, pcm or None, rate, bps, stats (candidates, chained, compacted), candidate records)"""
    lib = A._audio_lib()
    fn = lib.wh_flac_decode_frames
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                   C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int]
    ptr, n, ch, rate, bps = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    stats = (C.c_int32 * 4)()
    start, end = np.zeros(cand_cap, np.int64), np.zeros(cand_cap, np.int64)
    bs, status = np.zeros(cand_cap, np.int32), np.zeros(cand_cap, np.int32)
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    rc = fn(data, len(data), C.byref(ptr), C.byref(n), C.byref(ch), C.byref(rate), C.byref(bps), stats,
            start.ctypes.data_as(p64), bs.ctypes.data_as(p32), end.ctypes.data_as(p64), status.ctypes.data_as(p32), cand_cap)
    k = min(stats[0], cand_cap)
    records = dict(start=start[:k], bs=bs[:k], end=end[:k], rc=status[:k])
    if rc != 0:
        return rc, None, 0, 0, tuple(stats)[:3], records
    try:
        pcm = np.ctypeslib.as_array(ptr, shape=(n.value * ch.value,)).reshape(n.value, ch.value).copy()
    finally:
        lib.wh_flac_free(ptr)
    return 0, pcm, rate.value, bps.value, tuple(stats)[:3], records


MATRIX = [c[0] for c in fw.matrix()]


def case(name):
    return next(c for c in fw.matrix() if c[0] == name)


@pytest.mark.parametrize("name", MATRIX)
def test_writer_streams_decode_to_their_pcm(name):
    """guards the writer: the existing sequential decoder (CRCs and MD5 verified) returns the PCM the stream was made from"""
    _, data, pcm, rate, bps = case(name)
    got, r, b = A.decode_flac(data)
    assert (r, b) == (rate, bps) and got.dtype == np.int32 and np.array_equal(got, pcm)


def test_matrix_covers_what_it_claims():
    names = " ".join(MATRIX)
    for bs in (16, 192, 256, 1000, 4096, 65535):
        assert f"bs{bs}_" in names
    for frames in (1, 63, 64, 65, 130):
        assert f"_f{frames}_" in names
    for ch in (1, 2, 3, 8):
        assert f"_ch{ch}_" in names
    assert [len(fw.coded_number(v)) for v in (0, 200, 5000, 100000, 3000000, 100000000, 30000000000)] == [1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("name", MATRIX + ["jfk_head"])
def test_frames_route_equals_the_sequential_decoder(name):
    if name == "jfk_head":
        with open(JFK, "rb") as f:
            data = f.read()
    else:
        data = case(name)[1]
    want, rate, bps = A.decode_flac(data)
    rc, pcm, r, b, stats, rec = decode_frames(data)
    assert rc == 0 and (r, b) == (rate, bps)
    assert pcm.shape == want.shape and np.array_equal(pcm, want)
    assert stats[0] == stats[1] >= 1 and stats[2] == 0                # no false candidate: nothing to compact
    assert np.all(rec["rc"] == 0) and np.all(rec["end"][:-1] == rec["start"][1:])


@pytest.mark.parametrize("plants", [1, 40])
def test_planted_false_headers(plants):
    """complete frame headers (sync, consistent codes, CRC-8) inside a byte-aligned verbatim payload: candidates that the chain
    must leave out and the compaction must close up"""
    data, pcm, rate, bps = fw.planted(plants)
    rc, got, r, b, stats, rec = decode_frames(data)
    assert rc == 0
    candidates, chained, compacted = stats
    assert candidates == chained + plants and candidates > chained    # the case is not vacuous
    assert compacted == 1
    assert int(np.sum(rec["rc"] != 0)) == plants                      # every plant parsed garbage and failed its own checks
    want, _, _ = A.decode_flac(data)
    assert np.array_equal(got, want) and np.array_equal(got, pcm) and (r, b) == (rate, bps)


REJECTED = ["payload_byte", "header_byte", "cut_mid_frame", "chain_gap", "total_too_large"]


def fake_device_decoder(monkeypatch, calls):
    """stand in for the GPU: hip.flac_decode_device answered by the host twin, hip.resample by the host resampler's input"""
    def flac_decode_device(data, info):
        calls.append(info)
        rc, pcm, _, _, stats, _ = decode_frames(bytes(data.numpy().tobytes()))
        if rc != 0:
            return (hip.WH_ERR_LIMIT if rc == FLAC_E_UNSUP else hip.WH_ERR_STREAM), None, stats
        return 0, torch.from_numpy(pcm), stats
    monkeypatch.setattr(hip, "require_gpu", lambda device: None)
    monkeypatch.setattr(hip, "flac_decode_device", flac_decode_device)
    monkeypatch.setattr(hip, "resample", lambda pcm, rate, sr, bits=None: ("resampled", pcm.cpu().numpy().copy(), rate, bits))


@pytest.mark.parametrize("name", REJECTED)
def test_rejected_streams(name, tmp_path, monkeypatch):
    """the frames route returns its reject status; the Python route then surfaces the host decoder's own RuntimeError"""
    data = fw.rejections()[0][name]
    rc, pcm, *_ = decode_frames(data)
    assert rc == FLAC_E_REJECT and pcm is None
    with pytest.raises(RuntimeError) as host:
        A.decode_flac(data)
    path = tmp_path / f"{name}.flac"
    path.write_bytes(data)
    calls = []
    fake_device_decoder(monkeypatch, calls)
    with pytest.raises(RuntimeError) as routed:
        A.load_audio(str(path), device="cpu", decode_on_device=True)
    assert len(calls) == 1 and str(routed.value) == str(host.value)
    assert not isinstance(routed.value, hip.HipError)


def test_md5_is_the_one_difference():
    """a tampered MD5 alone: accepted by the frames route (it does not verify it), rejected by wh_flac_decode"""
    rej, good, pcm = fw.rejections()
    rc, got, *_ = decode_frames(rej["md5"])
    assert rc == 0 and np.array_equal(got, pcm)
    with pytest.raises(RuntimeError, match="MD5"):
        A.decode_flac(rej["md5"])
    assert np.array_equal(A.decode_flac(good)[0], pcm)


def test_what_the_route_does_not_take():
    pcm = fw.signal(600, 2, 32, seed=3)
    data32, _ = fw.encode_stream(pcm, 44100, 32, 256, assignment=lambda f: 10)        # 33-bit side channel
    assert np.array_equal(A.decode_flac(data32)[0], pcm)
    assert decode_frames(data32)[0] == FLAC_E_UNSUP
    unknown, _ = fw.encode_stream(fw.signal(600, 1, 16, seed=4), 44100, 16, 256, total=0)
    assert decode_frames(unknown)[0] == FLAC_E_UNSUP
    assert A.decode_flac(unknown)[0].shape == (600, 1)


def test_parse_flac_info_reads_what_the_decoder_reads():
    _, data, pcm, rate, bps = case("id3_padding_trailing")
    info = A.parse_flac_info(data)
    assert (info.sample_rate, info.channels, info.bits_per_sample, info.total_samples) == (rate, 2, bps, len(pcm))
    assert (info.min_block, info.max_block) == (3000 - 2 * 1152, 1152)
    assert data[info.first_frame: info.first_frame + 2] == b"\xff\xf8"
    _, _, _, _, _, rec = decode_frames(data)
    assert info.first_frame == rec["start"][0]
    assert A.parse_flac_info(b"RIFF" + bytes(40)) is None and A.parse_flac_info(data[:30]) is None


def test_routing(tmp_path, monkeypatch):
    """`device_ingest=True` and `load_audio(device=...)` without the flag never reach the new binding; "decode" and the flag
    do, and hand its PCM to the same hip.resample call"""
    _, data, pcm, rate, bps = case("assign10_short_last")
    path = tmp_path / "a.flac"
    path.write_bytes(data)
    calls = []
    fake_device_decoder(monkeypatch, calls)
    plain = A.load_audio(str(path), device="cpu")
    assert calls == [] and plain[0] == "resampled" and np.array_equal(plain[1], pcm)
    assert A.ingest_options(True) == {} and A.ingest_options(False) is None and A.ingest_options(0) is None
    assert A.ingest_options("decode") == {"decode_on_device": True}
    with pytest.raises(ValueError):
        A.ingest_options("gpu")
    flagged = A.load_audio(str(path), device="cpu", decode_on_device=True)
    assert len(calls) == 1 and calls[0].sample_rate == rate
    assert flagged[0] == "resampled" and np.array_equal(flagged[1], plain[1]) and flagged[2:] == plain[2:]

    # the entry points: what they ask of load_audio
    seen = []
    import sys
    T, AL = sys.modules["whisper_amd.transcribe"], sys.modules["whisper_amd.align"]    # (the package re-exports the functions)

    def spy(file, sr=16000, device=None, **kw):
        seen.append((device is not None, kw))
        raise RuntimeError("stop here")
    monkeypatch.setattr(T, "load_audio", spy)
    monkeypatch.setattr(AL, "load_audio", spy)

    class Model:
        device = "cpu"
    for flag, want in ((True, {}), ("decode", {"decode_on_device": True})):
        for call in (lambda: T.transcribe(Model(), str(path), device_ingest=flag),
                     lambda: T.transcribe_chunked(Model(), str(path), device_ingest=flag),
                     lambda: AL.align_batch(Model(), [str(path)], ["x"], device_ingest=flag)):
            seen.clear()
            with pytest.raises(RuntimeError, match="stop here"):
                call()
            assert seen == [(True, want)], (flag, seen)
    # the loader pool of transcribe_batch: `True` stages decoded PCM, "decode" stages the file itself
    monkeypatch.undo()
    calls = []
    fake_device_decoder(monkeypatch, calls)
    a = T._load_all([str(path), str(path)], torch.device("cpu"), False)
    assert calls == []
    b = T._load_all([str(path), str(path)], torch.device("cpu"), True)
    assert len(calls) == 2
    for x, y in zip(a, b):
        assert x[0] == y[0] == "resampled" and np.array_equal(x[1], y[1])
    for fn in (whisper_amd.transcribe_batch, whisper_amd.transcribe_chunked, whisper_amd.launcher.transcribe_sharded,
               whisper_amd.align_batch):
        assert inspect.signature(fn).parameters["device_ingest"].default is False
    assert inspect.signature(A.load_audio).parameters["decode_on_device"].default is False
