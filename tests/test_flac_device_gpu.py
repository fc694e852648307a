"""FLAC decoding on the GPU (csrc/flac.hip, wh_flac_decode_device, load_audio(..., decode_on_device=True)) against the host:
the candidate list and the per-candidate records against the host twin wh_flac_decode_frames, exactly; the PCM against the
sequential decoder wh_flac_decode, bit for bit; the statuses of tampered streams (the same bytes the sanitized host run of
tools/fuzz_flac_frames.c replays); load_audio and the file-level entry points with and without the device decoder."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import flac_writer as fw
import kernel_lib
import whisper_amd
from conftest import write_report
from test_flac_frames_cpu import JFK, MATRIX, REJECTED, case, decode_frames
from whisper_amd import audio as A
from whisper_amd import hip
from whisper_amd.synthetic import dims_for, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu

_P, _I, _L, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


def ktest():
    lib = kernel_lib.lib()
    lib.wht_flac_scratch_bytes.restype, lib.wht_flac_scratch_bytes.argtypes = _Z, [_Z, _I, _L, _I]
    lib.wht_flac_scan.restype, lib.wht_flac_scan.argtypes = _I, [_P, _Z, _Z, _I, _I, _I, _I, _L, _P, _P, _P, _P, _P, _P]
    lib.wht_flac_decode.restype, lib.wht_flac_decode.argtypes = _I, [_P, _Z, _I, _I, _I, _L, _P, _P, _P, _P, _P]
    return lib


def stream_bytes(name):
    if name == "jfk_head":
        with open(JFK, "rb") as f:
            return f.read()
    if name.startswith("planted"):
        return fw.planted(int(name[7:]))[0]
    return case(name)[1]


def device_records(data: bytes, dev, max_cand=2048):
    """scan + per-candidate decode through the wht_* hooks -> (n_found, start, bs, prov, end, rc, staging PCM)"""
    lib = ktest()
    info = A.parse_flac_info(data)
    staging = hip.flac_staging_frames(info.total_samples)
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    scratch = torch.empty(lib.wht_flac_scratch_bytes(len(data), info.channels, staging, max_cand), dtype=torch.uint8, device=dev)
    pcm = torch.zeros((staging, info.channels), dtype=torch.int32, device=dev)
    n = C.c_int(0)
    start, prov, end = (np.zeros(max_cand, np.int64) for _ in range(3))
    bs, rc = np.zeros(max_cand, np.int32), np.zeros(max_cand, np.int32)
    s = hip.stream_ptr(torch.cuda.current_stream(dev))
    assert lib.wht_flac_scan(d_file.data_ptr(), len(data), info.first_frame, info.channels, info.bits_per_sample, info.max_block,
                             max_cand, staging, scratch.data_ptr(), C.addressof(n), start.ctypes.data, bs.ctypes.data,
                             prov.ctypes.data, s) == 0
    assert 0 < n.value <= max_cand
    assert lib.wht_flac_decode(d_file.data_ptr(), len(data), info.channels, info.bits_per_sample, max_cand, staging,
                               pcm.data_ptr(), scratch.data_ptr(), end.ctypes.data, rc.ctypes.data, s) == 0
    k = n.value
    return k, start[:k], bs[:k], prov[:k], end[:k], rc[:k], pcm


def device_decode(data: bytes, dev):
    info = A.parse_flac_info(data)
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    return hip.flac_decode_device(d_file, info), info


ALL = MATRIX + ["jfk_head", "planted1", "planted40"]


@pytest.mark.parametrize("name", ALL)
def test_candidates_and_records_equal_the_host_twin(name, gpu_device):
    data = stream_bytes(name)
    _, _, _, _, stats, rec = decode_frames(data)
    k, start, bs, prov, end, rc, _ = device_records(data, gpu_device)
    assert k == stats[0]
    assert np.array_equal(start, rec["start"]) and np.array_equal(bs, rec["bs"])
    assert np.array_equal(prov, np.concatenate([[0], np.cumsum(rec["bs"])[:-1]]))
    assert np.array_equal(end, rec["end"]) and np.array_equal(rc, rec["rc"])


@pytest.mark.parametrize("name", ALL)
def test_device_pcm_equals_the_sequential_decoder(name, gpu_device):
    data = stream_bytes(name)
    want, rate, bps = A.decode_flac(data)
    (rc, pcm, stats), info = device_decode(data, gpu_device)
    assert rc == 0 and (info.sample_rate, info.bits_per_sample) == (rate, bps)
    assert pcm.dtype == torch.int32 and tuple(pcm.shape) == want.shape
    assert np.array_equal(pcm.cpu().numpy(), want)
    twin = decode_frames(data)[4]
    assert stats == twin                                              # candidates, chained frames, compacted: as the host twin
    if name.startswith("planted"):
        plants = int(name[7:])
        assert stats[0] == stats[1] + plants and stats[2] == 1        # the compaction ran
        write_report(f"flac_device_{name}.json", {"device": {"candidates": stats[0], "chained": stats[1]},
                                                  "host_twin": {"candidates": twin[0], "chained": twin[1]}})
    else:
        assert stats[0] == stats[1] and stats[2] == 0
    if name == "jfk_head":
        write_report("flac_device_jfk_head.json", {"device": {"candidates": stats[0], "chained": stats[1]},
                                                   "host_twin": {"candidates": twin[0], "chained": twin[1]}})


@pytest.mark.parametrize("name", REJECTED)
def test_rejected_streams_return_the_stream_status(name, gpu_device, tmp_path):
    """the five tampered inputs of the CPU test (replayed under sanitizers on the host first): a status, and the Python route
    then raises what the host decoder raises"""
    data = fw.rejections()[0][name]
    (rc, pcm, _), _ = device_decode(data, gpu_device)
    assert rc == hip.WH_ERR_STREAM and pcm is None
    path = tmp_path / "bad.flac"
    path.write_bytes(data)
    with pytest.raises(RuntimeError) as host:
        A.load_audio(str(path), device=gpu_device)
    with pytest.raises(RuntimeError) as routed:
        A.load_audio(str(path), device=gpu_device, decode_on_device=True)
    assert str(routed.value) == str(host.value)


def test_md5_is_not_verified_on_the_device(gpu_device):
    rej, good, pcm = fw.rejections()
    (rc, got, _), _ = device_decode(rej["md5"], gpu_device)
    assert rc == 0 and np.array_equal(got.cpu().numpy(), pcm)


def test_workspace_and_limit_statuses(gpu_device, tmp_path):
    data = case("assign10_short_last")[1]
    info = A.parse_flac_info(data)
    lib = hip.lib()
    staging, max_cand = hip.flac_staging_frames(info.total_samples), 1024
    need = lib.wh_flac_device_scratch_bytes(len(data), info.channels, staging, max_cand)
    assert need > 0 and lib.wh_flac_device_scratch_bytes(len(data), 9, staging, max_cand) == 0
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu_device)
    scratch = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    pcm = torch.empty((staging, info.channels), dtype=torch.int32, device=gpu_device)
    n = C.c_int64(0)
    s = hip.stream_ptr(torch.cuda.current_stream(gpu_device))

    def call(bits=info.bits_per_sample, scratch_bytes=need, total=info.total_samples, cand=max_cand):
        return lib.wh_flac_decode_device(d_file.data_ptr(), len(data), info.first_frame, info.channels, bits, info.max_block, total,
                                         pcm.data_ptr(), staging, cand, C.byref(n), None, scratch.data_ptr(), scratch_bytes, s)
    assert call(scratch_bytes=need - 1) == hip.WH_ERR_WORKSPACE        # one byte short
    assert call(bits=32) == hip.WH_ERR_LIMIT and call(total=0) == hip.WH_ERR_LIMIT
    assert call() == 0 and n.value == info.total_samples
    assert call(cand=2) == hip.WH_ERR_WORKSPACE                        # more candidates (4 frames) than the list holds
    # 32-bit FLAC: the Python route gives today's result
    pcm32 = fw.signal(3000, 2, 32, seed=3)
    path = tmp_path / "s32.flac"
    path.write_bytes(fw.encode_stream(pcm32, 44100, 32, 1024, assignment=lambda f: 10)[0])
    assert torch.equal(A.load_audio(str(path), device=gpu_device, decode_on_device=True), A.load_audio(str(path), device=gpu_device))


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000, "jfk"])
def test_load_audio_with_and_without_the_device_decoder(rate, gpu_device, tmp_path):
    if rate == "jfk":
        path = JFK
    else:
        pcm = fw.signal(20000, 2, 16 if rate != 48000 else 24, seed=rate)
        path = str(tmp_path / f"r{rate}.flac")
        with open(path, "wb") as f:
            f.write(fw.encode_stream(pcm, rate, 16 if rate != 48000 else 24, 4096, subs=fw.varied(), assignment=lambda f: 8 + f % 3)[0])
    calls = []
    real = hip.flac_decode_device

    def spy(data, info):
        out = real(data, info)
        calls.append(out[0])
        return out
    hip.flac_decode_device = spy
    try:
        plain = A.load_audio(path, device=gpu_device)
        assert calls == []
        flagged = A.load_audio(path, device=gpu_device, decode_on_device=True)
    finally:
        hip.flac_decode_device = real
    assert calls == [0]                                               # the device decoder ran and accepted the stream
    assert flagged.dtype == torch.float32 and flagged.device.type == "cuda" and torch.equal(flagged, plain)


def test_repeatability(gpu_device):
    data = fw.planted(40)[0]
    a, b = device_records(data, gpu_device), device_records(data, gpu_device)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:6], b[1:6]))
    (_, p1, s1), _ = device_decode(data, gpu_device)
    (_, p2, s2), _ = device_decode(data, gpu_device)
    assert s1 == s2 and torch.equal(p1, p2)


# ---- the file-level entry points ------------------------------------------------------------------------------------------
KW = dict(temperature=0.0, fp16=False, language="en", sample_len=12, no_speech_threshold=None, logprob_threshold=None,
          compression_ratio_threshold=None)


def same_result(a, b):
    assert a["text"] == b["text"] and a["language"] == b["language"] and len(a["segments"]) == len(b["segments"])
    for s, t in zip(a["segments"], b["segments"]):
        assert s["tokens"] == t["tokens"] and s["text"] == t["text"]
        assert (s["seek"], s["start"], s["end"]) == (t["seek"], t["start"], t["end"])
    assert a.get("chunks") == b.get("chunks")


def test_entry_points_decode_equals_true(gpu_device, tmp_path):
    """transcribe_chunked / transcribe_batch / transcribe under device_ingest="decode" == under device_ingest=True"""
    dims = dims_for("micro.en")
    ckpt = str(tmp_path / "micro.en.pt")
    save_checkpoint(ckpt, dims, synthetic_state_dict(dims, seed=1))
    model = whisper_amd.load_model(ckpt, device=gpu_device)
    synth = str(tmp_path / "s.flac")
    with open(synth, "wb") as f:
        f.write(fw.encode_stream(fw.signal(40000, 2, 16, seed=21), 8000, 16, 4096, subs=fw.varied())[0])
    paths = [JFK, synth]
    got = model.transcribe_batch(paths, batch_size=4, device_ingest="decode", **KW)
    want = model.transcribe_batch(paths, batch_size=4, device_ingest=True, **KW)
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        same_result(a, b)
    for p in paths:
        same_result(model.transcribe_chunked(p, batch_size=4, device_ingest="decode", **KW),
                    model.transcribe_chunked(p, batch_size=4, device_ingest=True, **KW))
    same_result(model.transcribe(JFK, device_ingest="decode", **KW), model.transcribe(JFK, device_ingest=True, **KW))
