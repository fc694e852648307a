#!/usr/bin/env python
"""bench.py — audio-seconds transcribed per wall-second on MI355X (BASELINE.json metric).

One "step" = one pass of the whole hot path over one batch of synthetic 30 s clips per GPU:
log-mel (HIP) -> AudioEncoder (MFMA) -> cross-KV -> greedy decode with the device-side sampling loop.
Workload at N=1 = BASELINE.json configs[2]: large-v3 dims, batch = 8 x 30 s, greedy, fp16.  The step
count is fixed: `sample_len` forced tokens per clip with EOT suppressed, so the work is
identical run to run.  Inputs are resident in HBM before the timed region.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]

--dump-outputs DIR writes what the timed path computed in its last step (the last decode chain of rank 0: token ids,
sum of log-probabilities and no-speech probability per row, what a caller of HipTask.greedy receives) as DIR/<name>.npy
in float64 / float32, so that two builds can be compared output for output on identical, seeded inputs.

Schedule (round 6): the K passes of --batch clips are COALESCED, --chain-batches (3) at a time, into decode chains of up to 24 rows —
one task, one prompt pass, one decode step per token for all of them, the decoder's weights streamed once per step for 24 clips
(whisper_amd.decode_many(chain_rows=24)) — and --in-flight (1) such chains run at once.  24 clips are resident at any time, as with
round 5's three 8-row lanes; `one_pass_at_a_time` is the same run's figure for one 8-row chain after the other.  Everything is driven
from ONE host thread (wh_task_greedy_begin + wh_task_poll when several chains are in flight).

N > 1: one process per GPU (the script re-executes itself under `torch.distributed.run` when it was not launched
by it), each rank decodes its own clips exactly as a single rank does (weak scaling, no collective in the step); rank 0 builds the
packed weight blob and RCCL-broadcasts it over xGMI at load.
Prints ONE JSON line on rank 0 (contract in the task statement).  Besides the headline it carries
  roofline      dominant kernel (cross-attention K/V stream) + `step_frac` of the whole decode step, HIP events
  public_api    the same workload through whisper_amd.log_mel_spectrogram + whisper_amd.decode (drop-in surface)
  parity        ALL rows x ALL sample_len steps of the timed pass against the oracle decoding the same 8 clips as one batch,
                token ids EXACT — the synthetic checkpoint is margin-conditioned on these clips first (oracle/condition.py:
                a trained model's peaked next-token distribution instead of the near-ties of random-init logits, on
                which no reduced-precision engine can be id-exact over 224 steps); the margins are reported
  extras        fp32_strict: the same workload on the fp32 strict-parity engine (logits within 1e-3 of the reference),
                audio-s/s + ids equal to the oracle —
                BASELINE configs[3] / [4] shaped workloads (beam 5; word timestamps) and configs[1] / [4] at their own
                model dims — never the headline; each leg carries its own roofline figures (decode-step fraction of
                the HBM peak, encoder TFLOP/s, log-mel time, device / host split of the alignment)
  cpu_baseline  the oracle (port of the reference's CPU fp32 path) on this box's host cores: one clip (warm-up +
                repeats) and the GPU's own batch of 8 clips (`value_batch8`, the figure the GPU / CPU ratio uses)

Weights: seeded random-init tensors of the named architecture, unless `--checkpoint PATH` is given or the released
checkpoint of `--model` sits in ~/.cache/whisper/ (where the reference's load_model keeps it): then those are used.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_T0 = time.perf_counter()


def log(msg: str) -> None:
    """progress to stderr (stdout carries exactly one JSON line)"""
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s float4-copy achievable)
MFMA_PEAK_TFLOPS = 2500.0   # dense fp16
# fp16 engine vs fp32 oracle at FULL depth (32 + 32 layers): max |dlogit| measured and asserted by
# tests/test_wide_gpu.py::test_large_v3_full_depth_vs_oracle (profiles/r03_parity_fp16.json)
FP16_FULL_DEPTH_MAX = 0.02
# port (oracle) vs the LIVE reference on the same host cores, time ratios (profiles/r03_calibrate_port.txt):
# the port is slightly FASTER than the reference, i.e. the CPU baseline errs on the CPU's side
PORT_CALIBRATION = {"port_time_over_reference_time": {"batch1_clip": 0.85, "batch8_clip": 0.92, "batch8_decode_step": 0.98},
                    "token_ids_equal": True, "source": "profiles/r03_calibrate_port.txt (tools/calibrate_port.py, build container, 8 threads)"}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--model", default="large-v3")
    p.add_argument("--batch", type=int, default=8, help="30 s clips per GPU")
    p.add_argument("--sample-len", type=int, default=224, help="forced decode steps per clip (n_text_ctx // 2)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-roofline", action="store_true")
    p.add_argument("--no-extras", action="store_true", help="skip the public-API leg and the beam / word-timestamp workloads")
    p.add_argument("--beam", type=int, default=5, help="beam size of the extra beam-search workload (0 = skip)")
    p.add_argument("--beam-steps", type=int, default=64)
    p.add_argument("--word-timestamps", dest="word_timestamps", action="store_true", default=True)
    p.add_argument("--no-word-timestamps", dest="word_timestamps", action="store_false")
    p.add_argument("--no-other-configs", dest="other_configs", action="store_false", default=True,
                   help="skip the base x 1 and turbo x 32 (+ word timestamps) legs of the extras")
    p.add_argument("--cpu-steps", type=int, default=12, help="decode steps timed on the CPU baseline")
    p.add_argument("--cpu-repeats", type=int, default=3)
    p.add_argument("--parity-steps", type=int, default=0, help="decode steps of the batch-8 oracle pass (parity of all rows); "
                                                               "0 = all sample_len steps")
    p.add_argument("--no-condition", action="store_true", help="plain seed-0 weights: no margin conditioning of the checkpoint "
                                                               "(the parity leg then reports near-ties instead of exact ids)")
    p.add_argument("--no-fp32-strict", action="store_true", help="skip the fp32 strict-parity engine leg of the extras")
    p.add_argument("--checkpoint", default=None, help="reference-format checkpoint to run instead of seeded weights "
                                                      "(default: ~/.cache/whisper/<model file> when it exists)")
    p.add_argument("--cpu-threads", type=int, default=0, help="host threads for the CPU baseline (0 = all usable cores)")
    p.add_argument("--task-form", type=int, default=0, help="developer A/B for chains of <= 8 rows: 0 = the default step (cross attention fused with its "
                                                           "query projection, csrc/xattn.hip), 1 = the self attention fused too (WH_TASK_FUSED_SELF), "
                                                           "2 = cross attention as two launches (the default with --in-flight > 1), 4 = keep the fused cross attention with --in-flight > 1")
    p.add_argument("--chain-batches", type=int, default=3, help="passes coalesced into one decode chain (rows of a chain = this x --batch; the row-tiled "
                                                                "projection kernels take up to 24 rows)")
    p.add_argument("--in-flight", type=int, default=1, help="decode chains in flight at once on this GPU, each on its own task and HIP stream, all driven "
                                                            "from one host thread; clips resident = --batch x --chain-batches x --in-flight")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64)")
    p.add_argument("--extras-in-flight", type=int, default=3, help="chains in flight in the `in_flight` variants of the extra legs (beam search, base x 1, turbo)")
    return p.parse_args()


def torchrun_command(n_gpus: int, argv, port: int):
    """argv + environment of `python bench.py --gpus N` re-executed as one process per GPU: the driver's own launch line
    (torch.distributed.run, one node, rendezvous on 127.0.0.1 — the container hostname may not resolve).  The
    environment is the caller's plus HSA_ENABLE_IPC_MODE_LEGACY=0 (the host driver only supports dmabuf IPC; without it
    RCCL fails with hipIpcGetMemHandle: invalid argument)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    return cmd, env


def relaunch_under_torchrun(args) -> None:
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run ... bench.py ...`"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd, env = torchrun_command(args.gpus, sys.argv[1:], port)
    log(f"--gpus {args.gpus} without a launcher: re-executing under torch.distributed.run (port {port})")
    os.execve(sys.executable, cmd, env)


def synth_audio(batch: int, rank: int, device) -> torch.Tensor:
    """seeded noise + three tones so the mel is not flat; clip index = global clip id."""
    n = 480000
    t = np.arange(n) / 16000.0
    clips = []
    for b in range(batch):
        rng = np.random.default_rng(rank * batch + b)
        x = rng.standard_normal(n).astype(np.float32) * 0.05
        for f, a in ((220.0 + 20 * b, 0.2), (1300.0, 0.1), (3100.0, 0.05)):
            x += (a * np.sin(2 * np.pi * f * t)).astype(np.float32)
        clips.append(x)
    return torch.from_numpy(np.stack(clips)).to(device)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    else:
        dist = None

    import faulthandler
    faulthandler.dump_traceback_later(300, repeat=True, file=sys.stderr)
    log(f"rank {rank}/{world} device ready")
    import whisper_amd
    from whisper_amd import hip
    from whisper_amd.audio import log_mel_spectrogram
    from whisper_amd.launcher import broadcast_weights
    from whisper_amd.model import ModelDimensions, Whisper
    from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict
    from whisper_amd.tokenizer import get_tokenizer

    ckpt_path = find_checkpoint(args)
    ckpt_sd = None
    if ckpt_path is not None:
        from types import SimpleNamespace
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        dims, ckpt_sd = SimpleNamespace(**ck["dims"]), ck["model_state_dict"]
        log(f"weights from checkpoint {ckpt_path}")
    else:
        dims = dims_for(args.model)
    dtype = hip.WH_F16
    want_cpu = rank == 0 and world == 1 and not args.no_cpu_baseline
    # ---- weights: rank 0 packs, everyone else receives the blob over RCCL -----------------------
    # With the CPU baseline the weights are generated on the host (numpy PCG64, bit-reproducible) so that the oracle and
    # the HIP engine see the very same tensors and their token ids can be compared; otherwise on the device (seconds).
    blob, sd_cpu, prep = None, None, None
    if rank == 0:
        if ckpt_sd is not None:
            sd_cpu = ckpt_sd
            if want_cpu:
                try:
                    prep = oracle_side(args, dims, sd_cpu, synth_audio(args.batch, rank, "cpu").numpy(), condition=False)
                except Exception as e:      # noqa: BLE001  (the headline never depends on the checker)
                    import traceback
                    traceback.print_exc(file=sys.stderr)
                    log(f"oracle side failed ({type(e).__name__}): no parity / batch CPU leg in this run")
                    prep = None
            blob = hip.pack_weights(sd_cpu, dims, dtype, device)
        elif want_cpu:
            sd_cpu = synthetic_state_dict(dims, seed=0, device="cpu")
            # the oracle's side of the parity leg runs FIRST: it conditions the synthetic checkpoint (token-embedding rows,
            # in place in sd_cpu) on this run's clips, then decodes them — what the timed HIP pass is compared with
            try:
                prep = oracle_side(args, dims, sd_cpu, synth_audio(args.batch, rank, "cpu").numpy(), condition=not args.no_condition)
            except Exception as e:      # noqa: BLE001  (the headline never depends on the checker)
                import traceback
                traceback.print_exc(file=sys.stderr)
                log(f"oracle side failed ({type(e).__name__}): no parity / batch CPU leg in this run")
                sd_cpu = synthetic_state_dict(dims, seed=0, device="cpu")
                prep = None
            blob = hip.pack_weights(sd_cpu, dims, dtype, device)
        else:
            sd = synthetic_state_dict(dims, seed=0, device=device)
            blob = hip.pack_weights(sd, dims, dtype, device)
            del sd
        torch.cuda.empty_cache()
    blob = broadcast_weights(blob, dims, dtype, device, dist)
    model = hip.HipModel(dims, dtype, blob)
    log(f"weights packed: {blob.numel() / 1e9:.2f} GB")

    B, N = args.batch, args.sample_len
    tok, init, suppress = token_setup(dims)              # suppressed ids include EOT: exactly N steps per clip
    T0 = len(init)
    mask = torch.zeros(dims.n_vocab, dtype=torch.uint8)
    mask[suppress] = 1
    mask = mask.to(device)
    params = hip.GreedyParams(sample_begin=T0, max_steps=N, n_ctx=dims.n_text_ctx, eot=tok.eot,
                              timestamp_begin=tok.timestamp_begin, no_timestamps=tok.no_timestamps,
                              max_initial_timestamp_index=50, suppress_blank=1,
                              blank_token=tok.encode(" ")[0], suppress_mask=mask.data_ptr())

    audio = synth_audio(B, rank, device)
    init_t = torch.tensor(init, device=device)
    sot_index = tok.sot_sequence.index(tok.sot)
    # ---- the schedule: chains of CB coalesced passes (CB x B rows each), F of them in flight, ONE host thread ------------------
    # A lane = a HIP stream + one task per chain shape on it (KV caches, step graphs) + its token buffers.  log-mel, encoder and
    # cross-K/V of a chain are enqueued on the lane's stream order (the encoder itself runs on the engine's stream with the engine's
    # one workspace); the decode loop is wh_task_greedy (F = 1) or wh_task_greedy_begin + wh_task_poll in turn (F > 1).
    sched = chain_schedule(args, world)
    CB, F, CR = sched["chain_batches"], sched["chains_in_flight"], sched["chain_rows"]      # CR: rows of a full chain
    # several chains in flight: no spinning kernel beside other chains (what HipModel.acquire_task gives a lane's task; --task-form 4
    # keeps the fused cross attention there for A/B)
    form = dict(fused_self=bool(args.task_form & 1), two_launch_cross=bool(args.task_form & 2) or (F > 1 and not args.task_form & 4))

    class Lane:
        def __init__(self, stream, form):
            self.stream, self.form = stream, form
            self.tasks, self.tokens = {}, {}

        def task(self, nb):
            if nb not in self.tasks:
                self.tasks[nb] = hip.HipTask(model, nb * B, 1, max(T0, 8), stream=self.stream, **self.form)
                self.tokens[nb] = torch.zeros(nb * B, T0 + N + 1, dtype=torch.int64, device=device)
            return self.tasks[nb], self.tokens[nb]

    lanes = [Lane(torch.cuda.Stream(device=device) if F > 1 else None, form) for _ in range(F)]
    for ln in lanes:
        ln.task(CB)
    if F > 1 and CB == 1:
        # the one-pass-at-a-time figure is ONE chain alone on the chip: the default step (fused cross attention), not a lane's
        serial_lane = Lane(lanes[0].stream, dict(fused_self=bool(args.task_form & 1), two_launch_cross=bool(args.task_form & 2)))
    else:
        serial_lane = lanes[0]
    serial_lane.task(1)                                   # the one-pass-at-a-time figure (and the tail chains of K % CB passes)
    torch.cuda.synchronize(device)

    def enqueue_chain(ln, nb, begin_only):
        """log-mel of every batch of the chain (its own clamp: audio.py:155), ONE encoder pass and ONE decode chain over all nb x B clips"""
        tk, toks = ln.task(nb)
        st = ln.stream if ln.stream is not None else torch.cuda.current_stream(device)
        with torch.cuda.stream(st):
            mels = [log_mel_spectrogram(audio, dims.n_mels) for _ in range(nb)]          # (B, n_mels, 3000) fp32 each
            feats = model.encode(mels[0] if nb == 1 else torch.cat(mels))
            tk.reset()
            tk.set_audio(feats)
            toks.zero_()
            toks[:, :T0] = init_t
            if begin_only:
                return tk.greedy_begin(toks, params, sot_index, tok.no_speech)
            return tk.greedy(toks, params, sot_index, tok.no_speech)

    last_chain = {}     # outputs of the last chain of the latest run_passes: token buffer + greedy's (n, sum_logprobs, no_speech_probs)

    def run_passes(k):
        """k passes of B clips as chains of up to CB passes, up to F chains in flight; returns the token count of the last chain"""
        sizes = [CB] * (k // CB) + ([k % CB] if k % CB else [])
        n = 0
        if F == 1:
            for nb in sizes:
                res = enqueue_chain(lanes[0], nb, False)
                n = res[0]
            last_chain.update(tokens=lanes[0].tokens[sizes[-1]], result=res)
            return n
        pend, nxt = [None] * F, 0
        while nxt < len(sizes) or any(p is not None for p in pend):
            for i in range(F):
                if pend[i] is None and nxt < len(sizes):
                    pend[i] = (enqueue_chain(lanes[i], sizes[nxt], True), nxt)
                    nxt += 1
                elif pend[i] is not None:
                    res = pend[i][0].poll()
                    if res is not None:
                        if pend[i][1] == len(sizes) - 1:
                            last_chain.update(tokens=lanes[i].tokens[sizes[-1]], result=res)
                        n, pend[i] = res[0], None
        return n

    def barrier():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(device)

    tail = args.steps % CB

    def timed_region():
        for w in range(args.warmup):
            run_passes(CB * F)
            if tail and w == 0:                     # the last chain of the timed region is shorter: its task and step graph exist before the clock starts
                for ln in lanes:
                    enqueue_chain(ln, tail, False)
            torch.cuda.synchronize(device)
            log("warmup pass done")
        barrier()
        t_start = time.perf_counter()
        n = run_passes(args.steps)
        barrier()
        return n, time.perf_counter() - t_start

    n_tok, elapsed = timed_region()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_chain, n_tok)
    per_rank_ms = [elapsed / args.steps * 1e3]
    if dist is not None:
        mine = torch.tensor([elapsed], dtype=torch.float64, device=device)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank_ms = [float(x.item()) / args.steps * 1e3 for x in every]     # imbalance shows here
        elapsed = max(float(x.item()) for x in every)                        # MAX over ranks
    assert n_tok == T0 + N, (n_tok, T0, N)
    ms_per_step = elapsed / args.steps * 1e3
    log(f"timed: {ms_per_step:.1f} ms per pass of {B} clips ({args.steps} passes as chains of {CR} rows, {F} in flight)")
    audio_s = 30.0 * B * world * args.steps
    value = audio_s / elapsed
    # the same passes ONE AT A TIME as chains of B rows (what rounds 1-4 reported as the headline), measured in the same run
    task, tokens = serial_lane.task(1)
    ks = max(2, min(args.steps, 6))
    enqueue_chain(serial_lane, 1, False)
    barrier()
    t0 = time.perf_counter()
    for _ in range(ks):
        enqueue_chain(serial_lane, 1, False)
    barrier()
    ser = (time.perf_counter() - t0) / ks
    serial = {"value": round(30.0 * B * world / ser, 2), "ms_per_step": round(ser * 1e3, 3), "steps": ks,
              "note": f"one pass of {B} clips after the other as chains of {B} rows on one task / stream; rank 0's clock"}
    log(f"one pass at a time: {ser * 1e3:.1f} ms per pass")
    direct_tokens = tokens[:, : T0 + N].clone()             # the B-row decode of the clips: what every group of B rows of a chain must equal
    chain_task, chain_tokens = lanes[0].task(CB)
    groups_equal, rows_eq, rows_all = None, 0, 0
    if args.steps >= CB:
        for ln in lanes[: max(1, min(F, (args.steps + CB - 1) // CB))]:
            for g in range(CB):
                eq = (ln.tokens[CB][g * B: (g + 1) * B, : T0 + N] == direct_tokens).all(dim=1)
                rows_eq, rows_all = rows_eq + int(eq.sum()), rows_all + B
        groups_equal = rows_eq == rows_all

    out = {
        "metric": "audio-seconds transcribed per wall-second (large-v3 greedy)",
        "value": round(value, 2), "unit": "audio-s/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f16",
        "data": ("synthetic" + (" (seeded random-init weights; cross-attention value biases and tied-embedding rows "
                                "margin-conditioned on these clips: oracle/condition.py)" if prep is not None and prep.get("conditioned") else ""))
                if ckpt_path is None else f"synthetic audio, weights of {os.path.basename(ckpt_path)}",
        "per_rank_ms_per_step": [round(x, 3) for x in per_rank_ms],
        "config": {"workload": f"{args.model} dims ({'random-init weights' if ckpt_path is None else 'released checkpoint'}), {B} x 30 s synthetic clips per pass, "
                               f"greedy, fp16 weights/KV + fp32 accumulate, {N} forced decode steps per clip "
                               f"(EOT suppressed), log-mel + encoder + cross-KV + decode timed; {CB} passes coalesced per decode chain "
                               f"({CR} rows: one task, the decoder's weights streamed once per step for all of them — whisper_amd.decode_many("
                               f"chain_rows={CR})), {F} chain(s) in flight, one host thread per GPU — one_pass_at_a_time is the same run's figure "
                               f"for chains of {B} rows one after the other",
                   "clips_per_gpu": B, "sample_len": N, "parallelism": f"dp{world} (clips sharded, no step collective)",
                   "chain_rows": CR, "chains_in_flight": F, "clips_resident": CR * F, "host_threads_per_gpu": 1},
        "clips_resident": CR * F,
        # every group of B rows of a chain decoded to exactly the ids the same B clips get as a chain of their own (the conditioned
        # checkpoint's margins are far above the fp16 engine's summation-order effects)
        "chain_groups_equal_one_pass_at_a_time": groups_equal,
        # (without the oracle's conditioning — --no-cpu-baseline, --gpus N — the weights are plain random-init: the top two logits then tie
        # to within fp16 rounding every few hundred steps and a 24-row chain, whose kernels sum in another order than an 8-row chain's,
        # may leave the 8-row decode at such a step; rows_equal counts the rows that did not)
        "chain_rows_equal_one_pass_at_a_time": {"rows_equal": rows_eq, "rows": rows_all,
                                                "checkpoint_conditioned": bool(prep is not None and prep.get("conditioned"))},
        "one_pass_at_a_time": serial,
    }

    # ---- roofline of the dominant kernels: HIP events on the launch stream, layer-rotated (HBM-cold) ----
    if rank == 0 and not args.no_roofline:
        kinds = {"decode_step": 0, "attn_decode_cross": 1, "attn_decode_self": 2, "gemv_qkv": 3, "gemv_fc1": 4, "gemv_fc2": 5,
                 "gemv_logits": 6, "gemv_out": 7}

        def kernel_table(tk, label):
            tab = {}
            for name, kind in kinds.items():
                ms, nbytes = tk.bench_kernel(kind, 64 if kind else 16)
                log(f"{label} kernel {name}: {ms * 1e3:.1f} us, {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s")
                tab[name] = {"avg_us": round(ms * 1e3, 2), "bytes": nbytes, "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1)}
            return tab
        kern = kernel_table(chain_task, f"{CR}-row chain")          # the timed schedule's chain
        kern8 = kernel_table(task, f"{B}-row chain") if CR != B else kern
        fused_cross = chain_task.fused_cross_attention
        # the MFMA-bound side of the pass, for orientation: AudioEncoder.forward on the batch (SURVEY.md §8d FLOP count)
        mel = log_mel_spectrogram(audio, dims.n_mels)
        model.encode(mel)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(3):
            model.encode(mel)
        torch.cuda.synchronize(device)
        enc_ms = (time.perf_counter() - t0) / 3 * 1e3
        enc_flop = encoder_flop(dims, B)
        kern["encoder_forward"] = {"avg_us": round(enc_ms * 1e3, 1), "flop": enc_flop, "clips": B,
                                   "TFLOPs": round(enc_flop / (enc_ms * 1e-3) / 1e12, 1), "mfma_peak_TFLOPs": MFMA_PEAK_TFLOPS,
                                   "frac": round(enc_flop / (enc_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}
        log(f"encoder forward: {enc_ms:.1f} ms, {enc_flop / (enc_ms * 1e-3) / 1e12:.0f} TFLOP/s")
        dom = kern["attn_decode_cross"]
        # HBM traffic per launch from the PMC counters: they cannot be read from inside this process, so the
        # figure comes from the committed rocprofv3 --pmc passes of this same command (profiles/, per round),
        # and only when it was taken on this very workload (model, rows of the chain); otherwise null.
        traffic, tsrc = None, None
        for rnd in ("r06", "r05", "r04", "r03"):
            tf = os.path.join(ROOT, "profiles", f"{rnd}_pmc_traffic.json")
            if os.path.isfile(tf) and args.model == "large-v3":
                with open(tf) as f:
                    pj = json.load(f)
                pm = pj["kernels"].get("attn_decode_cross")
                if pm and int(pj.get("rows", 8)) == CR:
                    traffic = pm["hbm_read_bytes_corrected"] + pm["hbm_write_bytes_raw"]
                    tsrc = (f"profiles/{rnd}_pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 gfx950 correction + "
                            "WRITE_SIZE raw, bytes per launch)")
                    break
        step, step8 = kern["decode_step"], kern8["decode_step"]
        dom_name = ("xattn8_kernel (cross-attention K/V stream with LayerNorm + query projection inside the launch)"
                    if fused_cross else f"attn_decode_kernel<half> (cross-attention K/V stream of the {CR} rows of a chain)")
        n_chains = (args.steps + CB - 1) // CB
        out["roofline"] = {"bound": "hbm", "kernel": dom_name,
                           "achieved": dom["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(dom["GBps"] / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
                           "bytes_per_launch": dom["bytes"], "avg_us": dom["avg_us"], "rows": CR,
                           # the whole decode step of a chain (all dependent launches of one token) against the same peak
                           "step_frac": round(step["GBps"] / HBM_PEAK_GBS, 4), "step_avg_us": step["avg_us"],
                           "step_bytes": step["bytes"], "all_kernels": kern,
                           "measured_as": f"every kernel and the step of a {CR}-row chain alone on the chip (HIP events on its launch stream, "
                                          "layer-rotated); profiles/r06_kernel_stats.csv is the kernel trace of the same command",
                           # the timed region itself: the chains' decode steps against the HBM peak (algorithmic bytes: the weights ONCE per
                           # chain step; the encoder's share of a pass is MFMA work)
                           "pass_level": {"chains_in_flight": F, "chain_rows": CR, "decode_bytes_per_chain": step["bytes"] * N,
                                          "GBps": round(step["bytes"] * N * n_chains / elapsed / 1e9, 1),
                                          "frac": round(step["bytes"] * N * n_chains / elapsed / 1e9 / HBM_PEAK_GBS, 4)},
                           # the same figures for ONE chain of B rows (the kernels of rounds 3-5: fused cross attention launch)
                           "one_chain_b8": {"kernel": "xattn8_kernel" if task.fused_cross_attention else "attn_decode_kernel<half>",
                                            "achieved": kern8["attn_decode_cross"]["GBps"],
                                            "frac": round(kern8["attn_decode_cross"]["GBps"] / HBM_PEAK_GBS, 4),
                                            "avg_us": kern8["attn_decode_cross"]["avg_us"], "bytes_per_launch": kern8["attn_decode_cross"]["bytes"],
                                            "step_avg_us": step8["avg_us"], "step_bytes": step8["bytes"],
                                            "step_frac": round(step8["GBps"] / HBM_PEAK_GBS, 4), "all_kernels": kern8}}
    tf_err = None
    if rank == 0 and prep is not None:
        try:
            tf_err = teacher_forced_logit_error(model, model.encode(log_mel_spectrogram(audio, dims.n_mels)), prep, T0)
            log(f"teacher-forced fp16 logit error along the oracle's path: max {tf_err['max_abs_dlogit']:.4f} rms {tf_err['rms_dlogit']:.5f}")
        except Exception as e:      # noqa: BLE001  (a checker leg: never at the price of the line)
            import traceback
            traceback.print_exc(file=sys.stderr)
            tf_err = {"error": f"{type(e).__name__}: {e}"[:200]}
    if rank == 0:
        # fused step kernels: bounded spins that ran out / loops re-run on the two-launch kernels because of them, over ALL lanes
        # (must be 0: with several chains on the chip a producer workgroup may be dispatched late, the bounds have to hold there too)
        out["handoff_timeouts"] = sum(t.handoff_timeouts() for ln in lanes for t in ln.tasks.values())
        out["handoff_fallbacks"] = sum(t.handoff_fallbacks for ln in lanes for t in ln.tasks.values())
    for ln in lanes + ([serial_lane] if serial_lane is not lanes[0] else []):
        for t in ln.tasks.values():
            t.close()
        ln.tasks.clear()
        ln.tokens.clear()
    if F > 1:
        model.adopt_lane_streams([ln.stream for ln in lanes])      # the public-API legs below run their lanes on the same streams

    # ---- the same workload through the public drop-in surface ----------------------------------------------------
    if rank == 0 and world == 1 and not args.no_extras:      # single-GPU runs only: the scaling runs stay short
        try:
            wmodel = Whisper(ModelDimensions(**dims_dict(dims)), {}, device=device)
            wmodel.adopt_engine(torch.float16, model)
            opts = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=N, suppress_tokens=[-1, tok.eot])

            def api_pass():
                mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
                return whisper_amd.decode(wmodel, mel, opts)

            res = api_pass()
            torch.cuda.synchronize(device)
            same = all(r.tokens == direct_tokens[i, T0:].tolist() for i, r in enumerate(res))
            # the headline's schedule through the public surface: `reps` batches of raw audio, coalesced into chains of CR rows, F
            # chains in flight (decode_many).  First use in the process: one untimed call of one chain per lane (tasks, step graphs)
            reps = max(CB * F, min(args.steps, 4 * CB * F)) // (CB * F) * (CB * F)
            whisper_amd.decode_many(wmodel, [audio] * (CB * F), opts, in_flight=F, chain_rows=CR)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            many = whisper_amd.decode_many(wmodel, [audio] * reps, opts, in_flight=F, chain_rows=CR)
            torch.cuda.synchronize(device)
            same = same and all(r.tokens == direct_tokens[i, T0:].tolist() for rs in many for i, r in enumerate(rs))
            path = (f"whisper_amd.decode_many(model, [audio batch of {B}] * {reps}, DecodingOptions(fp16=True, sample_len=N), "
                    f"in_flight={F}, chain_rows={CR})")
            api_ms = (time.perf_counter() - t0) / reps * 1e3
            out["public_api"] = {"ms_per_step": round(api_ms, 3), "vs_direct": round(api_ms / ms_per_step, 4),
                                 "tokens_equal_direct": bool(same), "path": path}
            log(f"public API leg: {api_ms:.1f} ms per pass ({api_ms / ms_per_step:.3f} x direct), tokens equal: {same}")

            extras = {}
            EF = max(1, args.extras_in_flight)
            # the headline is N = 224 (worst case); N = 64 is the speech-typical length of a 30 s window
            if N != 64:
                o64 = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=64, suppress_tokens=[-1, tok.eot])

                def pass64():
                    return whisper_amd.decode(wmodel, whisper_amd.log_mel_spectrogram(audio, dims.n_mels), o64)

                pass64()
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for _ in range(3):
                    pass64()
                torch.cuda.synchronize(device)
                ms64 = (time.perf_counter() - t0) / 3 * 1e3
                extras["greedy_sample_len_64"] = {"clips": B, "steps": 64, "ms_per_pass": round(ms64, 2),
                                                  "audio_s_per_s": round(B * 30.0 / (ms64 / 1e3), 1),
                                                  "path": "whisper_amd.decode (public API), log-mel + encoder + 64 forced steps"}
                whisper_amd.decode_many(wmodel, [audio] * (CB * F), o64, in_flight=F, chain_rows=CR)
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                whisper_amd.decode_many(wmodel, [audio] * (3 * CB * F), o64, in_flight=F, chain_rows=CR)
                torch.cuda.synchronize(device)
                l64 = (time.perf_counter() - t0) / (3 * CB * F) * 1e3
                extras["greedy_sample_len_64"]["coalesced"] = {"chain_rows": CR, "chains_in_flight": F, "ms_per_pass": round(l64, 2),
                                                               "audio_s_per_s": round(B * 30.0 / (l64 / 1e3), 1), "passes": 3 * CB * F}
                log(f"greedy, 64 steps: {ms64:.1f} ms per pass = {B * 30.0 / (ms64 / 1e3):.0f} audio-s/s")
            # NOT the headline (BASELINE configs[2] fixes 8 clips per batch; the headline keeps 24 clips resident as round 5 did): what the
            # same engine does when MORE clips are pending — two / three 24-row chains in flight (48 / 72 clips resident), one host thread
            if args.model == "large-v3" and B == 8 and CR == 24:
                more = {}
                for nf in (2, 3):
                    whisper_amd.decode_many(wmodel, [audio] * (3 * nf), opts, in_flight=nf, chain_rows=24)
                    torch.cuda.synchronize(device)
                    t0 = time.perf_counter()
                    many = whisper_amd.decode_many(wmodel, [audio] * (6 * nf), opts, in_flight=nf, chain_rows=24)
                    torch.cuda.synchronize(device)
                    mms = (time.perf_counter() - t0) / (6 * nf) * 1e3
                    more[f"{24 * nf}_clips_resident"] = {
                        "chains_in_flight": nf, "chain_rows": 24, "ms_per_pass": round(mms, 2), "audio_s_per_s": round(30.0 * B / (mms * 1e-3), 1),
                        "passes": 6 * nf, "tokens_equal_direct": all(r.tokens == direct_tokens[i, T0:].tolist() for rs in many for i, r in enumerate(rs))}
                    log(f"{24 * nf} clips resident ({nf} chains of 24 rows in flight): {mms:.1f} ms per pass = {30.0 * B / (mms * 1e-3):.0f} audio-s/s")
                extras["more_clips_resident"] = more
            # BASELINE configs[3] shape: beam search (beam 5) on this GPU's clips, device-side beam loop
            if args.beam >= 2:
                bopts = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=args.beam_steps, beam_size=args.beam,
                                                    suppress_tokens=[-1, tok.eot])
                mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
                whisper_amd.decode(wmodel, mel, bopts)
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for _ in range(2):
                    mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
                    bres = whisper_amd.decode(wmodel, mel, bopts)
                torch.cuda.synchronize(device)
                bms = (time.perf_counter() - t0) / 2 * 1e3
                extras["beam_search"] = {"beam_size": args.beam, "clips": B, "rows": B * args.beam, "steps": args.beam_steps,
                                         "ms_per_pass": round(bms, 2), "audio_s_per_s": round(30.0 * B / (bms * 1e-3), 1)}
                if EF > 1:
                    # B x beam rows per pass is more than a 24-row chain takes: the passes stay chains of their own, EF in flight
                    mel_b = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
                    whisper_amd.decode_many(wmodel, [mel_b] * EF, bopts, in_flight=EF)
                    torch.cuda.synchronize(device)
                    t0 = time.perf_counter()
                    many = whisper_amd.decode_many(wmodel, [audio] * (2 * EF), bopts, in_flight=EF)
                    torch.cuda.synchronize(device)
                    lms = (time.perf_counter() - t0) / (2 * EF) * 1e3
                    extras["beam_search"]["in_flight"] = {
                        "passes_in_flight": EF, "ms_per_pass": round(lms, 2), "audio_s_per_s": round(30.0 * B / (lms * 1e-3), 1),
                        "passes": 2 * EF, "host_threads": 1,
                        "winners_equal_to_one_at_a_time": all([r.tokens for r in rs] == [r.tokens for r in bres] for rs in many)}
                    log(f"beam {args.beam}, {EF} passes in flight: {lms:.1f} ms per pass")
                bp = beam_parity(bres, prep, "fp16")
                if bp is not None:
                    extras["beam_search"]["parity"] = bp
                    log(f"beam {args.beam} parity vs oracle: winners equal {bp['winners_equal']} of {bp['clips']}")
                # the 40-row decode step alone (graph replay, HIP events) at the pass's middle position, against its
                # algorithmic bytes (weights once + every audio's cross K/V once + the rows' self K/V + logits)
                extras["beam_search"].update(step_roofline(model, model.encode(mel), B, args.beam, T0 + args.beam_steps // 2))
                log(f"beam {args.beam}: {bms:.1f} ms per pass of {B} clips x {args.beam_steps} steps")
            # the headline model's decode step at 16 and 20 rows (9 - 24 rows run on gemv8_kernel's row tiles since round 5)
            if args.model == "large-v3" and B == 8:
                f8 = model.encode(whisper_amd.log_mel_spectrogram(audio, dims.n_mels))
                extras["step_at_other_row_counts"] = {
                    "16_rows": step_roofline(model, torch.cat([f8, f8]).contiguous(), 16, 1, T0 + 32),
                    "4x5_beam_rows": step_roofline(model, f8[:4].contiguous(), 4, 5, T0 + 32)}
                log(f"decode step at 16 rows: {extras['step_at_other_row_counts']['16_rows']['step_us']} us, "
                    f"at 4 x 5 beam rows: {extras['step_at_other_row_counts']['4x5_beam_rows']['step_us']} us")
            # BASELINE configs[4] shape: word timestamps (cross-attention alignment + DTW) for every clip of the batch
            if args.word_timestamps:
                from whisper_amd.timing import find_alignment_batch
                mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
                text = [[t for t in r.tokens if t < tok.eot][:200] for r in res]
                find_alignment_batch(wmodel, tok, text, mel.half(), [3000] * B)
                torch.cuda.synchronize(device)
                stats, wts = {}, []
                for _ in range(5):          # every call listed; the figure is their MEAN (round 4 reported a median of three over a
                    t0 = time.perf_counter()   # bimodal leg: the score slabs now live in the cached task, whisper_amd/hip.py)
                    al = find_alignment_batch(wmodel, tok, text, mel.half(), [3000] * B, stats=stats)
                    torch.cuda.synchronize(device)
                    wts.append((time.perf_counter() - t0) * 1e3)
                wms = sum(wts) / len(wts)
                extras["word_timestamps"] = {"clips": B, "text_tokens_per_clip": len(text[0]), "ms_per_batch": round(wms, 2),
                                             "calls_ms": [round(x, 1) for x in wts],
                                             "calls_spread": round((max(wts) - min(wts)) / min(wts), 4),
                                             "words": sum(len(a) for a in al),
                                             # wall clock until the device results (paths, probabilities) are on the host /
                                             # host-only work after that (word split, boundaries), last batch
                                             "device_ms": round(stats.get("device_s", 0.0) * 1e3, 2),
                                             "host_ms": round(stats.get("host_s", 0.0) * 1e3, 2),
                                             "host_share": round(stats.get("host_s", 0.0) / max(stats.get("device_s", 0.0) + stats.get("host_s", 0.0), 1e-9), 3),
                                             "note": "find_alignment_batch: encoder + one teacher-forced pass + alignment heads QK + DTW"}
                log(f"word timestamps: {wms:.1f} ms per batch of {B} clips")
            # the tolerance-meeting engine on the same workload: fp32 strict parity (reference operation order, logits within
            # 1e-3 of the fp32 reference — tests/test_wide_gpu.py), timed the same way, ids against the same oracle decode
            if not args.no_fp32_strict and sd_cpu is not None:
                extras["fp32_strict"] = fp32_strict_leg(dims, sd_cpu, device, audio, B, N, T0, init, params, tok, prep, args)
            out["extras"] = extras
            out["flags"] = {"public_api_within_5pct_of_direct": bool(out["public_api"]["vs_direct"] <= 1.05),
                            "word_timestamps_calls_spread_below_10pct": (bool(extras["word_timestamps"]["calls_spread"] <= 0.1)
                                                                         if "word_timestamps" in extras else None)}
            wmodel = None
            # BASELINE configs[1] (base, 1 clip, greedy) and configs[4] (turbo, 32 clips, greedy + word timestamps) at their own
            # model dims, through the public API; weights generated on the device
            if args.other_configs and args.model == "large-v3":
                task_bytes = model.task_cache_bytes
                model.drop_cached_tasks()
                extras["other_configs"] = other_configs(device, N, EF, check=want_cpu, log_=log)
                model.task_cache_bytes = task_bytes
        except Exception as e:      # the optional legs never cost the headline line: report and go on
            import traceback
            traceback.print_exc(file=sys.stderr)
            out.setdefault("extras", {})["error"] = f"{type(e).__name__}: {e}"[:300]

    # ---- CPU baseline: the oracle (fp32 torch-CPU restatement of the reference) on this box's host cores ----
    if want_cpu:
        try:
            base, parity = cpu_baseline(args, dims, init, suppress, tok, audio.cpu().numpy(), sd_cpu,
                                        direct_tokens[:, T0:].cpu().tolist(), prep)
            base["gpu_over_cpu_batch8"] = round(value / base["value_batch8"], 1) if base.get("value_batch8") else None
            base["calibration"] = PORT_CALIBRATION
            out["cpu_baseline"] = base
            if parity is not None and tf_err is not None:
                # the id check alone cannot see numeric drift below the conditioned margins (>= 0.35): the measured logit error
                # of the timed engine on THIS checkpoint and these clips stands beside it, against the asserted full-depth bound
                parity["teacher_forced_logits"] = tf_err
                parity["numerics_ok"] = bool(parity["tokens_equal"] and tf_err.get("within_bound", False))
            out["parity"] = parity
        except Exception as e:          # never at the price of the measured line
            import traceback
            traceback.print_exc(file=sys.stderr)
            out["cpu_baseline"] = {"value": None, "error": f"{type(e).__name__}: {e}"[:300]}

    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()                      # rank 0 measures its kernel table after the timed region: leave together
        dist.destroy_process_group()


def dump_outputs(out_dir: str, last_chain: dict, n_tok: int) -> None:
    """--dump-outputs: the last timed chain's results as .npy (token ids exact in float64; a few KB in all)"""
    toks = last_chain["tokens"][:, :n_tok].cpu().numpy().astype(np.float64)
    _, sum_lp, nsp = last_chain["result"]
    arrays = {"tokens": toks, "sum_logprobs": sum_lp.cpu().numpy().astype(np.float32)}
    if nsp is not None:
        arrays["no_speech_probs"] = nsp.cpu().numpy().astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    log(f"outputs of the last timed step: {', '.join(f'{k} {v.shape}' for k, v in arrays.items())} -> {out_dir}")


def chain_schedule(args, world: int) -> dict:
    """How a rank cuts its passes into decode chains.  A function of the command line ONLY — never of the number of ranks or of
    the host's core count: every rank of `--gpus N` runs exactly what `--gpus 1` runs (one host thread per rank drives all its
    chains; round 5 capped the lanes per rank by usable cores // world, so an 8-rank run did less per GPU than the 1-rank line
    it was compared with).  tests/test_launcher_gloo.py checks it across world sizes."""
    del world
    cb, f = max(1, int(args.chain_batches)), max(1, int(args.in_flight))
    return {"chain_batches": cb, "chains_in_flight": f, "chain_rows": cb * int(args.batch),
            "clips_resident": cb * int(args.batch) * f, "host_threads": 1}


def token_setup(dims):
    """tokenizer, initial tokens and the suppressed ids of the fixed-length greedy workload (EOT suppressed: exactly
    sample_len steps per clip)"""
    from whisper_amd.tokenizer import get_tokenizer
    multilingual = dims.n_vocab >= 51865
    tok = get_tokenizer(multilingual, num_languages=dims.n_vocab - 51765 - int(multilingual), language="en", task="transcribe")
    suppress = sorted(set(list(tok.non_speech_tokens) + [tok.transcribe, tok.translate, tok.sot, tok.sot_prev,
                                                         tok.sot_lm, tok.no_speech, tok.eot]))
    return tok, list(tok.sot_sequence), suppress


def oracle_rules(dims, tok, init, suppress):
    import oracle
    return oracle.SamplingRules(sample_begin=len(init), sot_index=0, eot=tok.eot, n_ctx=dims.n_text_ctx,
                                timestamp_begin=tok.timestamp_begin, no_timestamps=tok.no_timestamps,
                                suppress_tokens=suppress, blank_token=tok.encode(" ")[0], no_speech=tok.no_speech)


def oracle_side(args, dims, sd, audio_np, condition: bool) -> dict:
    """The CHECKER's half of the parity leg, run before any HIP work (it is also the batch-B leg of the CPU baseline, so
    every stage is timed): the oracle (fp32 port of the reference's CPU path, SDPA attention) computes log-mel and
    encoder output of this run's B clips as one batch, optionally margin-conditions the synthetic checkpoint on them
    (oracle/condition.py — the decoder's cross-attention value biases and token-embedding rows edited IN PLACE in `sd`,
    before the engines are packed from it), then
    greedy-decodes all sample_len (or --parity-steps) steps with the plain oracle: the tokens every row of the timed HIP
    pass must equal, the filtered logits they were chosen from, and the decision margins."""
    import oracle
    from oracle import condition as cond
    from whisper_amd.utils import usable_cores
    cores = getattr(args, "cpu_threads", 0) or usable_cores()
    torch.set_num_threads(cores)
    tok, init, suppress = token_setup(dims)
    rules = oracle_rules(dims, tok, init, suppress)
    om = oracle.OracleModel(dims, sd, sdpa=True)
    filt = oracle.mel_filterbank(dims.n_mels)
    B = audio_np.shape[0]
    n_steps = args.parity_steps if args.parity_steps > 0 else args.sample_len
    log(f"oracle side: {args.model} fp32 on {cores} host threads, {B} clips x {n_steps} steps" + (", conditioning" if condition else ""))
    with torch.no_grad():
        t0 = time.perf_counter()
        mels = torch.stack([oracle.log_mel_spectrogram(audio_np[b], filt) for b in range(B)])
        t_mel = time.perf_counter() - t0
        om.encoder(mels[:1])                     # warm-up (thread pool, allocator, first-touch of the 2.5 GB of fp32 weights)
        t0 = time.perf_counter()
        feats = om.encoder(mels)
        t_enc = time.perf_counter() - t0
        log(f"oracle side: log-mel {t_mel:.2f}s, encoder {t_enc:.1f}s (after a one-clip warm-up)")
        built, t_cond = None, 0.0
        backup = None
        if condition:
            t0 = time.perf_counter()
            # what the conditioning edits, kept so that a failure leaves the plain seeds behind (never at the price of the line)
            backup = {k: v.clone() for k, v in sd.items()
                      if k == cond.EMB or k.endswith(".cross_attn.value.bias")}
            try:
                # (1) the random-init encoder's output is one constant vector plus a little (cos 0.999 between clips): cancel
                # its contribution to the cross-attention values (value biases), or the decoder cannot tell steps and rows
                # apart; (2) margin-condition the tied embedding along the greedy decode of these clips
                c = cond.center_cross_values(om, feats)
                log(f"oracle side: cross-attention value biases centred on the clips' mean encoder output (|c| = {float(c.norm()):.1f} "
                    f"of |x| = {float(feats.norm(dim=-1).mean()):.1f})")
                # the first --beam-steps decisions carry margins of 2 - 4 logits, so that the beam-search leg (which runs over
                # exactly those steps on this same checkpoint) is decided by the model, not by which host computes the oracle
                head = (args.beam_steps, 2.0, 4.0) if getattr(args, "beam", 0) >= 2 and not args.no_extras else None
                built = cond.condition_greedy(om, feats, init, n_steps, rules, seed=0, margin=(0.35, 3.0), log=log, passes=2, head=head)
            except Exception as e:      # noqa: BLE001
                log(f"oracle side: conditioning failed ({type(e).__name__}: {e}) - plain seed weights, near-tie rule")
                for k, v in backup.items():
                    sd[k].copy_(v)
                built, condition = None, False
            backup = None
            t_cond = time.perf_counter() - t0
        # the CHECKER's decode (keeps every step's filtered logits, walks the timestamp rule twice per row): untimed
        dec = oracle.greedy_decode(om, feats, init, n_steps, rules, keep_logits=True)
        # the CPU BASELINE's batch leg: the plain decode, warm (the conditioning passes / the decode above ran these shapes)
        t0 = time.perf_counter()
        plain = oracle.greedy_decode(om, feats, init, n_steps, rules)
        t_dec = time.perf_counter() - t0
        assert torch.equal(plain["tokens"], dec["tokens"])
        # the beam-search leg's reference (BASELINE configs[3] shape): every clip's candidates and ranked winner
        beam = None
        if getattr(args, "beam", 0) >= 2 and not args.no_extras:
            t0 = time.perf_counter()
            bd = oracle.beam_decode(om, feats, init, args.beam_steps, rules, args.beam)
            def gap(c):      # the oracle winner's own separation from its runner-up hypothesis (all candidates have equal length here)
                sc = sorted((lp / max(len([t for t in toks[len(init):] if t != tok.eot]), 1) for toks, lp in c), reverse=True)
                return sc[0] - sc[1] if len(sc) > 1 else float("inf")
            beam = {"winners": [oracle.decoding.rank_candidates(c, len(init), tok.eot) for c in bd["candidates"]],
                    "gaps": [gap(c) for c in bd["candidates"]],
                    "steps": args.beam_steps, "beam": args.beam, "t": time.perf_counter() - t0}
            log(f"oracle side: beam {args.beam} x {args.beam_steps} steps of {B} clips in {beam['t']:.1f}s")
    mg = cond.margins_of(dec)
    consistent = built is None or bool(torch.equal(built["tokens"], dec["tokens"]))
    log(f"oracle side: decode {t_dec:.1f}s ({t_dec / n_steps * 1e3:.0f} ms/step incl. the prompt pass), margins {mg}"
        + ("" if consistent else "  [conditioning pass and plain decode DISAGREE]"))
    return {"dec": dec, "steps": n_steps, "t_mel": t_mel, "t_enc": t_enc, "t_dec": t_dec, "t_cond": t_cond, "margins": mg,
            "conditioned": bool(condition), "consistent": consistent, "cores": cores, "beam": beam,
            "edited_rows": 0 if built is None else len(built["rows"])}


def find_checkpoint(args):
    """--checkpoint PATH, else the released checkpoint of --model where the reference's load_model keeps it
    (~/.cache/whisper/<file>, whisper/__init__.py:126-135), else None (seeded random-init weights)"""
    if args.checkpoint:
        if not os.path.isfile(args.checkpoint):
            raise SystemExit(f"--checkpoint {args.checkpoint}: no such file")
        return args.checkpoint
    from whisper_amd.registry import MODEL_URLS
    url = MODEL_URLS.get(args.model)
    if url is None:
        return None
    default = os.path.join(os.path.expanduser("~"), ".cache")
    path = os.path.join(os.getenv("XDG_CACHE_HOME", default), "whisper", os.path.basename(url))
    return path if os.path.isfile(path) else None


def encoder_flop(dims, B: int) -> float:
    """AudioEncoder.forward on B windows: two convolutions + per layer 12 D^2 per frame of projections
    and MLP (x 2 flop) + 4 T^2 D of attention"""
    D_, L_, M_ = dims.n_audio_state, dims.n_audio_layer, dims.n_mels
    return float(B) * (2 * 3000 * M_ * 3 * D_ + 2 * 1500 * D_ * 3 * D_ + L_ * (24 * 1500 * D_ * D_ + 4 * 1500 * 1500 * D_))


def beam_parity(res, prep, engine):
    """The ranked winner of every clip of a HIP beam-search pass (DecodingResult list) against the oracle's
    BeamSearchDecoder + MaximumLikelihoodRanker restatement on the same clips (oracle_side: decoding.py:301-404, 190-213):
    token sequences equal — no near-tie rule — and the winners' sum_logprobs side by side."""
    if prep is None or not prep.get("beam"):
        return None
    want = prep["beam"]["winners"]
    rows = []
    for a, (r, (body, lp)) in enumerate(zip(res, want)):
        got_lp = r.avg_logprob * (len(r.tokens) + 1)
        rows.append({"clip": a, "equal": r.tokens == list(body), "oracle_norm_score_gap_to_runner_up": round(prep["beam"]["gaps"][a], 4),
                     "first_divergence": None if r.tokens == list(body) else next((i for i, (x, y) in enumerate(zip(r.tokens, body)) if x != y), min(len(r.tokens), len(body))),
                     "sum_logprob": round(got_lp, 4), "oracle_sum_logprob": round(lp, 4)})
    n_eq = sum(x["equal"] for x in rows)
    return {"engine": engine, "clips": len(rows), "beam": prep["beam"]["beam"], "steps": prep["beam"]["steps"],
            "winners_equal": n_eq, "tokens_equal": n_eq == len(rows),
            "max_sum_logprob_err": round(max(abs(x["sum_logprob"] - x["oracle_sum_logprob"]) for x in rows if x["equal"]), 4) if n_eq else None,
            "per_clip": rows, "checkpoint_conditioned": bool(prep.get("conditioned")),
            # a clip whose ORACLE winner leads its own runner-up by less than this (length-normalised log-probability) is a
            # coin toss between two fp32 hosts already; such a clip is listed, never counted as equal
            "mismatches_where_the_oracle_itself_is_a_near_tie": sum((not x["equal"]) and x["oracle_norm_score_gap_to_runner_up"] < 0.3 / prep["beam"]["steps"] for x in rows),
            "rule": "ranked winner of every clip (token ids) EXACTLY the oracle's; no near-tie rule"}


def fp32_strict_leg(dims, sd_cpu, device, audio, B, N, T0, init, params, tok, prep, args=None) -> dict:
    """BASELINE configs[2] workload on the fp32 strict-parity engine (WH_F32: the reference's operation order, fp32 weights,
    activations and K/V, exact-fp32 MFMA / FMA chains): log-mel + encoder + cross-KV + N greedy steps, 1 warm-up + 2 timed
    passes; its token ids against the oracle's decode of the same clips (all rows, all steps).  Then BASELINE configs[3]'s
    shape (beam search) on the same engine — the engine that meets north_star's beam tolerance (logits within 1e-3)."""
    import whisper_amd
    from whisper_amd import hip
    from whisper_amd.audio import log_mel_spectrogram
    from whisper_amd.model import ModelDimensions, Whisper
    from whisper_amd.synthetic import dims_dict
    eng = hip.HipModel(dims, hip.WH_F32, hip.pack_weights(sd_cpu, dims, hip.WH_F32, device))
    task = hip.HipTask(eng, B, 1, max(T0, 8))
    tokens = torch.zeros(B, T0 + N + 1, dtype=torch.int64, device=device)
    init_t = torch.tensor(init, device=device)
    sot_index = tok.sot_sequence.index(tok.sot)
    try:
        def one():
            feats = eng.encode(log_mel_spectrogram(audio, dims.n_mels))
            task.reset()
            task.set_audio(feats)
            tokens.zero_()
            tokens[:, :T0] = init_t
            return task.greedy(tokens, params, sot_index, tok.no_speech)[0]
        one()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(2):
            n = one()
        torch.cuda.synchronize(device)
        ms = (time.perf_counter() - t0) / 2 * 1e3
        res = {"dtype": "f32", "ms_per_pass": round(ms, 2), "audio_s_per_s": round(30.0 * B / (ms * 1e-3), 1), "steps": N,
               "engine": "WH_F32 strict parity (logits within 1e-3 of the fp32 reference: tests/test_wide_gpu.py)"}
        st_ms, st_bytes = task.bench_kernel(0, 8)
        res.update({"step_us": round(st_ms * 1e3, 1), "step_bytes": st_bytes,
                    "step_frac": round(st_bytes / (st_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
        if prep is not None:
            rows = tokens[:, T0: T0 + N].cpu().tolist()
            par = parity_report(prep["dec"], init, rows, prep["steps"], prep, engine="fp32 strict")
            res["parity"] = {k: par[k] for k in ("rows", "steps", "rows_equal", "rows_near_tie", "rows_wrong", "tokens_equal")}
        log(f"fp32 strict engine: {ms:.1f} ms per pass = {res['audio_s_per_s']} audio-s/s, step {res['step_us']} us, "
            f"ids equal to the oracle: {res.get('parity', {}).get('tokens_equal')}")
        if args is not None and args.beam >= 2:
            task.close()
            wm = Whisper(ModelDimensions(**dims_dict(dims)), {}, device=device)
            wm.adopt_engine(torch.float32, eng)
            bopts = whisper_amd.DecodingOptions(language="en", fp16=False, sample_len=args.beam_steps, beam_size=args.beam,
                                                suppress_tokens=[-1, tok.eot])

            def bpass():
                return whisper_amd.decode(wm, whisper_amd.log_mel_spectrogram(audio, dims.n_mels), bopts)
            bres = bpass()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(2):
                bres = bpass()
            torch.cuda.synchronize(device)
            bms = (time.perf_counter() - t0) / 2 * 1e3
            bb = {"beam_size": args.beam, "clips": B, "rows": B * args.beam, "steps": args.beam_steps,
                  "ms_per_pass": round(bms, 2), "audio_s_per_s": round(30.0 * B / (bms * 1e-3), 1)}
            bb.update(step_roofline(eng, eng.encode(log_mel_spectrogram(audio, dims.n_mels)), B, args.beam, T0 + args.beam_steps // 2))
            bp = beam_parity(bres, prep, "fp32 strict")
            if bp is not None:
                bb["parity"] = {k: bp[k] for k in ("clips", "winners_equal", "tokens_equal", "max_sum_logprob_err")}
            res["beam_search"] = bb
            log(f"fp32 strict engine, beam {args.beam}: {bms:.1f} ms per pass, step {bb['step_us']} us, winners equal: "
                f"{bb.get('parity', {}).get('winners_equal')}")
            wm = None
        return res
    finally:
        task.close()
        eng.drop_cached_tasks()
        del eng
        torch.cuda.empty_cache()


def teacher_forced_logit_error(engine, feats, prep, T0: int, n_steps: int = 8) -> dict:
    """The timed engine's raw logits along the ORACLE's own greedy path (prompt pass + n_steps single-token steps, all rows)
    against the oracle's filtered fp32 logits of the same positions, on the entries the filters left finite (they only
    write -inf: decoding.py:423-505).  Unlike the id check this sees drift well below the conditioned margins.  The HIP side
    runs its own log-mel + fp16 encoder, so the figure includes the encoder's error."""
    from whisper_amd import hip
    dec = prep["dec"]
    n_steps = min(n_steps, len(dec["step_logits"]) - 1)
    B = feats.shape[0]
    toks = dec["tokens"][:, : T0 + n_steps].to(feats.device)
    task = hip.HipTask(engine, B, 1, max(T0, 8))
    worst, sq, cnt, per_pos = 0.0, 0.0, 0, []
    try:
        task.set_audio(feats.contiguous())
        got = [task.prefill(toks[:, :T0].contiguous())[:, -1].float().cpu()]
        for i in range(T0, T0 + n_steps):
            got.append(task.step(toks[:, i].contiguous()).float().cpu())
    finally:
        task.close()
    for i, g in enumerate(got):
        want = dec["step_logits"][i].float()
        ok = torch.isfinite(want)
        d = (g - want)[ok].abs()
        per_pos.append(round(float(d.max()), 5))
        worst = max(worst, float(d.max()))
        sq += float((d.double() ** 2).sum())
        cnt += int(ok.sum())
    bound = 2.0 * FP16_FULL_DEPTH_MAX
    return {"rows": B, "positions": len(got), "max_abs_dlogit": round(worst, 5), "rms_dlogit": round((sq / max(cnt, 1)) ** 0.5, 6),
            "per_position_max": per_pos, "bound": bound, "within_bound": bool(worst < bound),
            "note": f"bound = 2 x the full-depth fp16 bound asserted by tests/test_wide_gpu.py on shared features ({FP16_FULL_DEPTH_MAX}; observed here 0.020 - 0.028); "
                    "here the engine also runs its own fp16 encoder on the audio"}


def step_roofline(engine, feats, B: int, G: int, position: int) -> dict:
    """One decode step of R = B x G rows at `position` cached tokens: the captured step graph replayed and timed with HIP
    events on the launch stream (wh_task_bench_kernel kind 0), against its algorithmic bytes — every weight matrix and
    the tied logits matrix once, every audio's cross K/V once, the rows' self K/V, the logits written."""
    from whisper_amd import hip
    dims = engine.dims
    task = hip.HipTask(engine, B, G, 64 if position <= 64 else dims.n_text_ctx)
    try:
        task.set_audio(feats.contiguous())
        g = torch.Generator(device=feats.device).manual_seed(1)
        toks = torch.randint(0, dims.n_vocab - 1600, (B * G, position), generator=g, device=feats.device)
        task.prefill(toks, sel=[position - 1])
        ms, nbytes = task.bench_kernel(0, 16)
    finally:
        task.close()
    gbps = nbytes / (ms * 1e-3) / 1e9
    return {"step_us": round(ms * 1e3, 1), "step_bytes": nbytes, "step_rows": B * G, "step_position": position,
            "step_GBps": round(gbps, 1), "step_frac": round(gbps / HBM_PEAK_GBS, 4)}


def event_ms(fn, device, reps: int = 5) -> float:
    """median device time of fn() between two events on the current stream"""
    fn()
    torch.cuda.synchronize(device)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def other_configs(device, N, in_flight=3, check=False, log_=log, head=32):
    """BASELINE.json configs[1] / configs[4] shapes on this GPU (never the headline): audio-s/s through
    log_mel_spectrogram + decode() [+ find_alignment_batch], fixed N steps per clip, synthetic weights of those dims.
    check: every leg carries a `parity` object — the weights are then generated on the host, margin-conditioned by the oracle on the
    leg's first clips over the first `head` decisions (oracle/condition.py build_reference: oracle log-mel -> oracle encoder -> greedy
    decode), and the first `head` token ids of those clips in the TIMED configuration's result must equal the oracle's."""
    import whisper_amd
    from whisper_amd import hip
    from whisper_amd.model import ModelDimensions, Whisper
    from whisper_amd.synthetic import dims_dict, dims_for, synthetic_state_dict
    from whisper_amd.timing import find_alignment_batch
    from whisper_amd.tokenizer import get_tokenizer
    res = {}
    for name, batch, words in (("base", 1, False), ("turbo", 32, True)):
        dims = dims_for(name)
        audio = synth_audio(batch, 0, device)
        ref, n_ref = None, min(batch, 4)
        if check:
            try:
                from oracle import condition
                t0 = time.perf_counter()
                sd = synthetic_state_dict(dims, seed=0, device="cpu")
                tok_, init_, suppress_ = token_setup(dims)
                rules_ = oracle_rules(dims, tok_, init_, suppress_)
                ref = condition.build_reference(dims, sd, audio[:n_ref].cpu().numpy(), init_, head, rules_, seed=3)
                ref["T0"] = len(init_)
                log_(f"other config {name}: oracle conditioned {n_ref} clip(s) x {head} steps in {time.perf_counter() - t0:.1f}s, margins {ref['margins']}")
            except Exception as e:      # noqa: BLE001 — never at the price of the leg
                import traceback
                traceback.print_exc(file=sys.stderr)
                ref = {"error": f"{type(e).__name__}: {e}"[:200]}
                sd = synthetic_state_dict(dims, seed=0, device=device)
        else:
            sd = synthetic_state_dict(dims, seed=0, device=device)
        eng = hip.HipModel(dims, hip.WH_F16, hip.pack_weights(sd, dims, hip.WH_F16, device))
        del sd
        m = Whisper(ModelDimensions(**dims_dict(dims)), {}, device=device)
        m.adopt_engine(torch.float16, eng)
        tok = get_tokenizer(True, num_languages=dims.n_vocab - 51765 - 1, language="en", task="transcribe")
        opts = whisper_amd.DecodingOptions(language="en", fp16=True, sample_len=N, suppress_tokens=[-1, tok.eot])

        def one():
            mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
            r = whisper_amd.decode(m, mel, opts)
            if words:
                text = [[t for t in x.tokens if t < tok.eot][:200] for x in r]
                find_alignment_batch(m, tok, text, mel.half(), [3000] * batch,
                                     audio_features=torch.stack([x.audio_features for x in r]))   # as transcribe() does
            return r
        one()
        one()                               # two warm-up passes: the first timed pass was still 1.5-2 x slower after one
        torch.cuda.synchronize(device)
        times = []
        for _ in range(3):                  # median of three passes (a 54 ms pass is easily disturbed by a host hiccup)
            t0 = time.perf_counter()
            last = one()
            torch.cuda.synchronize(device)
            times.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(times)[1]
        key = f"{name}_x{batch}" + ("_word_timestamps" if words else "")
        res[key] = {"ms_per_pass": round(ms, 2), "audio_s_per_s": round(30.0 * batch / (ms * 1e-3), 1), "steps": N,
                    "passes_ms": [round(x, 1) for x in times]}
        log(f"other config {key}: {ms:.1f} ms per pass = {30.0 * batch / (ms * 1e-3):.0f} audio-s/s")
        if ref is not None and "dec" in ref:
            T0_ = ref["T0"]
            want = ref["dec"]["tokens"][:, T0_: T0_ + head].tolist()
            rows = [{"clip": i, "equal": last[i].tokens[:head] == want[i],
                     "first_divergence": next((j for j, (x, y) in enumerate(zip(last[i].tokens[:head], want[i])) if x != y), None)}
                    for i in range(n_ref)]
            res[key]["parity"] = {"engine": "fp16", "clips_checked": n_ref, "of_clips": batch, "steps": head,
                                  "rows_equal": sum(r_["equal"] for r_ in rows), "tokens_equal": all(r_["equal"] for r_ in rows),
                                  "per_clip": rows, "oracle_margins": ref["margins"], "conditioning_consistent": ref["consistent"],
                                  "rule": f"the first {head} token ids of the first {n_ref} clip(s) of the timed pass EXACTLY the oracle's (oracle log-mel + "
                                          f"encoder + greedy decode of those clips; checkpoint margin-conditioned on them over these {head} decisions)"}
            log(f"other config {key}: parity vs oracle {res[key]['parity']['rows_equal']} of {n_ref} clips over {head} steps")
        elif ref is not None:
            res[key]["parity"] = ref
        if in_flight > 1:
            # the same passes, `in_flight` at once (run_in_lanes: a host thread + HIP stream per pass; the threads sleep while they wait)
            from whisper_amd.decoding import run_in_lanes
            reps = 2 * in_flight
            run_in_lanes(m, [one] * in_flight, in_flight, torch.float16)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run_in_lanes(m, [one] * reps, in_flight, torch.float16)
            torch.cuda.synchronize(device)
            lms = (time.perf_counter() - t0) / reps * 1e3
            res[key]["in_flight"] = {"passes_in_flight": in_flight, "ms_per_pass": round(lms, 2),
                                     "audio_s_per_s": round(30.0 * batch / (lms * 1e-3), 1), "passes": reps}
            log(f"other config {key}, {in_flight} passes in flight: {lms:.1f} ms per pass = {30.0 * batch / (lms * 1e-3):.0f} audio-s/s")
        if batch == 1:
            # 24 one-clip requests coalesced into ONE 24-row chain (decode_many(chain_rows=24)): the weights once per step for all
            many_in = [audio] * 24
            whisper_amd.decode_many(m, many_in, opts, in_flight=1, chain_rows=24)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            got = whisper_amd.decode_many(m, many_in, opts, in_flight=1, chain_rows=24)
            torch.cuda.synchronize(device)
            cms = (time.perf_counter() - t0) / 24 * 1e3
            res[key]["coalesced"] = {"chain_rows": 24, "ms_per_pass": round(cms, 2), "audio_s_per_s": round(30.0 / (cms * 1e-3), 1),
                                     "passes": 24, "tokens_equal_one_at_a_time": all(g[0].tokens == last[0].tokens for g in got)}
            log(f"other config {key}, 24 requests as one 24-row chain: {cms:.2f} ms per clip = {30.0 / (cms * 1e-3):.0f} audio-s/s")
        # where this leg stands against the hardware: log-mel, encoder (MFMA peak), one decode step (HBM peak)
        mel = whisper_amd.log_mel_spectrogram(audio, dims.n_mels)
        mel_ms = event_ms(lambda: whisper_amd.log_mel_spectrogram(audio, dims.n_mels), device)
        enc_ms = event_ms(lambda: eng.encode(mel), device, reps=3)
        flop = encoder_flop(dims, batch)
        res[key].update({"mel_us": round(mel_ms * 1e3, 1), "encoder_ms": round(enc_ms, 3),
                         "encoder_TFLOPs": round(flop / (enc_ms * 1e-3) / 1e12, 1),
                         "encoder_frac": round(flop / (enc_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)})
        res[key].update(step_roofline(eng, eng.encode(mel), batch, 1, 4 + N // 2))
        log(f"other config {key}: mel {mel_ms * 1e3:.0f} us, encoder {res[key]['encoder_TFLOPs']} TFLOP/s, "
            f"step {res[key]['step_us']} us = {res[key]['step_frac']} of HBM peak")
        eng.drop_cached_tasks()
        m = eng = None
        torch.cuda.empty_cache()
    return res


def cpu_baseline(args, dims, init, suppress, tok, audio_np, sd, hip_rows, prep=None):
    """Oracle = "port": same algorithm as the reference's CPU fp32 path, attention through
    scaled_dot_product_attention as the reference's default (model.py:124-128); calibrated beside the live reference in
    BASELINE.md §2b.  Bounded sample, two legs on the same workload:
      batch 1  — clip 0: log-mel + encoder, one warm-up and `cpu_repeats` timed repetitions; decode runs of k and 2k
                 steps -> `value`;
      batch B  — all clips as ONE batch, as the reference's decode() can (decoding.py:713-789) and as the GPU pass runs:
                 the encoder once, one run of `parity_steps` steps (its tokens are what every HIP row is compared with;
                 it also warms this shape up), then runs of k / 2 and 3k / 2 steps -> `value_batch8`, the fair side of
                 the GPU / CPU ratio (the 6 GB fp32 weight read of a step is shared by the rows).
    A decode run of n steps costs  fixed + n * step  (fixed = the prompt pass incl. the cross-attention K/V projection of
    all 32 layers, paid once per clip): two run lengths give both, and the clip is extrapolated as
    log-mel + encoder + fixed + sample_len * step.
    `hip_rows`: the sampled tokens of every row of the timed HIP pass (same weights, same clips), or None.
    `prep`: the result of `oracle_side` (run before the HIP work): its batch-B encoder and FULL-length decode are the batch
    leg — measured end to end over all steps, nothing extrapolated — and its tokens are the parity reference."""
    import oracle
    from whisper_amd.utils import usable_cores
    cores = getattr(args, "cpu_threads", 0) or usable_cores()
    torch.set_num_threads(cores)
    log(f"cpu_baseline: {args.model} fp32 oracle on {cores} host threads")
    om = oracle.OracleModel(dims, sd, sdpa=True)
    filt = oracle.mel_filterbank(dims.n_mels)
    reps = max(1, args.cpu_repeats)
    B = audio_np.shape[0]
    N = args.sample_len

    def timed(fn, n):
        fn()                                       # warm-up (thread pool, allocator, caches)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return r, ts

    def once(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    rules = oracle.SamplingRules(sample_begin=len(init), sot_index=0, eot=tok.eot, n_ctx=dims.n_text_ctx,
                                 timestamp_begin=tok.timestamp_begin, no_timestamps=tok.no_timestamps,
                                 suppress_tokens=suppress, blank_token=tok.encode(" ")[0], no_speech=tok.no_speech)

    def decode_cost(feats, n_short, n_long, reps_):
        """(fixed seconds per run, seconds per step) from runs of two lengths, medians of reps_ repetitions"""
        ts, tl = [], []
        for _ in range(reps_):
            ts.append(once(lambda: oracle.greedy_decode(om, feats, init, n_short, rules))[1])
            tl.append(once(lambda: oracle.greedy_decode(om, feats, init, n_long, rules))[1])
        step = (statistics.median(tl) - statistics.median(ts)) / (n_long - n_short)
        return max(statistics.median(ts) - n_short * step, 0.0), step, ts, tl

    mel, t_mel = timed(lambda: oracle.log_mel_spectrogram(audio_np[0], filt), reps)
    with torch.no_grad():
        feats, t_enc = timed(lambda: om.encoder(mel[None]), reps)
        k = max(args.cpu_steps, 2)
        oracle.greedy_decode(om, feats, init, 2, rules)                     # warm-up of the decode shapes
        fixed1, step1, ts1, tl1 = decode_cost(feats, k, 2 * k, reps)
    m_mel, m_enc = statistics.median(t_mel), statistics.median(t_enc)
    total = m_mel + m_enc + fixed1 + step1 * N
    log(f"cpu_baseline: log-mel {m_mel:.3f}s encoder {m_enc:.2f}s prompt pass {fixed1:.2f}s step {step1 * 1e3:.0f} ms (x{reps})")
    lo = 30.0 / (max(t_mel) + max(t_enc) + fixed1 + (max(tl1) - min(ts1)) / k * N)
    hi = 30.0 / (min(t_mel) + min(t_enc) + fixed1 + max(min(tl1) - max(ts1), 1e-9) / k * N)
    base = {"value": round(30.0 / total, 3), "unit": "audio-s/s", "cores": cores, "kind": "port",
            "repeats": reps, "spread": [round(min(lo, hi), 3), round(max(lo, hi), 3)],
            "sample": f"1 clip of the same workload, 1 warm-up + {reps} repeats, medians: log-mel {m_mel:.3f}s + encoder "
                      f"{m_enc:.2f}s + prompt pass (incl. cross K/V) {fixed1:.2f}s + {step1 * 1e3:.0f} ms/step (from runs of "
                      f"{k} and {2 * k} steps), extrapolated to {N} steps (fp32, torch CPU, SDPA attention, {cores} threads)"}
    if B == 1:
        return base, None
    # ---- the GPU's own batch: B clips in one oracle batch
    if prep is not None:
        kp, decB = prep["steps"], prep["dec"]
        # every stage measured by oracle_side; a decode shorter than sample_len is extended by its own per-step time
        stepB = prep["t_dec"] / kp
        totalB = prep["t_mel"] + prep["t_enc"] + prep["t_dec"] + (N - kp) * stepB
        base["value_batch8"] = round(30.0 * B / totalB, 3)
        base["batch8"] = {"clips": B, "logmel_s": round(prep["t_mel"], 2), "encoder_s": round(prep["t_enc"], 2),
                          "decode_s": round(prep["t_dec"], 2), "decode_steps": kp,
                          "ms_per_step_incl_prompt_pass": round(stepB * 1e3, 1),
                          "sample": f"{B} clips as one batch, measured end to end: log-mel {prep['t_mel']:.2f}s + encoder "
                                    f"{prep['t_enc']:.1f}s + greedy decode of {kp} steps {prep['t_dec']:.1f}s"
                                    + ("" if kp == N else f", extended to {N} steps at {stepB * 1e3:.0f} ms/step")}
        log(f"cpu_baseline batch {B}: encoder {prep['t_enc']:.1f}s, decode {prep['t_dec']:.1f}s -> {base['value_batch8']} audio-s/s")
    else:
        kp = max(args.parity_steps if args.parity_steps > 0 else 24, 1)
        with torch.no_grad():
            mels, t_melB = once(lambda: torch.stack([oracle.log_mel_spectrogram(audio_np[b], filt) for b in range(B)]))
            featsB, t_encB = once(lambda: om.encoder(mels))
            decB, t_first = once(lambda: oracle.greedy_decode(om, featsB, init, kp, rules, keep_logits=True))
            k2 = max(k // 2, 2)
            fixedB, stepB, tsB, tlB = decode_cost(featsB, k2, 3 * k2, 1)
        totalB = t_melB + t_encB + fixedB + stepB * N
        base["value_batch8"] = round(30.0 * B / totalB, 3)
        base["batch8"] = {"clips": B, "encoder_s": round(t_encB, 2), "prompt_pass_s": round(fixedB, 2),
                          "ms_per_step": round(stepB * 1e3, 1), "first_run_s": round(t_first, 2),
                          "sample": f"{B} clips as one batch: log-mel {t_melB:.2f}s + encoder {t_encB:.1f}s (once) + prompt pass "
                                    f"{fixedB:.2f}s + {stepB * 1e3:.0f} ms/step (runs of {k2} and {3 * k2} steps after a "
                                    f"{kp}-step first run), extrapolated to {N} steps"}
        log(f"cpu_baseline batch {B}: encoder {t_encB:.1f}s, prompt pass {fixedB:.2f}s, {stepB * 1e3:.0f} ms/step -> "
            f"{base['value_batch8']} audio-s/s")
    if hip_rows is None:                       # tools/cpu_baseline_only.py: no HIP pass to compare with
        return base, None
    # ---- parity of the benchmarked engine: every row of the timed HIP pass against the oracle's tokens for that clip
    parity = parity_report(decB, init, hip_rows, kp, prep)
    log(f"parity vs oracle ({B} rows x {kp} steps): equal {parity['rows_equal']}, near-tie {parity['rows_near_tie']}, "
        f"wrong {parity['rows_wrong']}")
    return base, parity


def parity_report(decB, init, hip_rows, kp, prep=None, engine="fp16") -> dict:
    """every row of a HIP pass against the oracle's decode of the same clips: ids equal over all `kp` steps, or where they
    first differ and by what margin in the oracle's own filtered logits (a near-tie only counts as such on the plain
    random-init checkpoint, where it is unavoidable; on the margin-conditioned checkpoint any difference is `wrong`)"""
    import oracle
    B = len(hip_rows)
    conditioned = bool(prep and prep.get("conditioned"))
    bound = 0.0 if conditioned else 2 * FP16_FULL_DEPTH_MAX
    rows, n_eq, n_tie = [], 0, 0
    for b in range(B):
        want = decB["tokens"][b, len(init):].tolist()
        got = hip_rows[b][: len(want)]
        t = oracle.first_divergence(got, want)
        row = {"row": b, "first_divergence": t, "margin": None}
        if t is None:
            n_eq += 1
        else:
            lg = decB["step_logits"][t][b]
            m = float(lg[want[t]]) - float(lg[got[t]])
            row["margin"] = round(m, 5) if np.isfinite(m) else None        # a filtered-out token has no finite margin
            row["near_tie"] = bool(np.isfinite(m) and 0 <= m < bound)
            n_tie += int(row["near_tie"])
        rows.append(row)
    rep = {"engine": engine, "rows": B, "steps": kp, "rows_equal": n_eq, "rows_near_tie": n_tie,
           "rows_wrong": B - n_eq - n_tie, "tokens_equal": n_eq == B, "per_row": rows}
    if prep is not None:
        rep["checkpoint"] = ("seed-0 weights; cross-attention value biases centred on the clips' mean encoder output and "
                             f"{prep['edited_rows']} tied-embedding rows margin-conditioned on these clips (oracle/condition.py)"
                             if conditioned else "as given (no conditioning)")
        rep["oracle_margins"] = prep["margins"]
        rep["conditioning_consistent"] = prep["consistent"]
    rep["rule"] = (f"{engine} engine vs fp32 oracle, all {B} rows x {kp} steps: token ids EXACT (no near-tie rule; the oracle's "
                   "own top-1 margins are in oracle_margins)" if conditioned else
                   f"{engine} engine vs fp32 oracle, all {B} rows x {kp} steps: ids equal, or the first difference of a row is a "
                   f"near-tie (< {bound} = twice the measured full-depth fp16 logit bound) in the oracle's filtered logits")
    return rep


if __name__ == "__main__":
    main()
