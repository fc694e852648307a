"""The decode step of 9 - 24 rows with LayerNorm behind the MFMAs (csrc/kernels.h) against the same step with the LayerNorm
prologue everywhere (WH_TASK_LN_PROLOGUE), in one process: D = 384, 4 + 4 layers, 17 and 24 rows, 32 steps.  At this width
both one-slot LayerNorm projections of a layer (cross query, FC1) take the new form.

The two forms agree to rounding, not bit for bit, and on seeded random-init weights the top two of ~50 000 logits lie hundredths
apart somewhere in every few hundred decisions (oracle/condition.py), so "token ids equal" would test the weights, not the
kernels.  The checkpoint is therefore margin-conditioned as in test_wide_gpu.py's token-exact tests (every greedy decision of the
fp32 oracle wins by >= 0.3, asserted), and then
  * the device-side greedy decode gives the SAME token ids with and without the flag — and they are the oracle's;
  * host-driven steps, teacher-forced along that path, give logits that differ by no more than 6e-2, the tolerance
    test_wide_gpu.py's step tests hold the fp16 engine to at these widths;
  * the prefill is bit-identical (it is not touched)."""
import pytest
import torch

import oracle
from oracle import condition
from whisper_amd import hip

pytestmark = pytest.mark.gpu

N_STEPS, ROWS_MAX = 32, 24


@pytest.fixture(scope="module")
def conditioned(gpu_device):
    from whisper_amd.tokenizer import get_tokenizer
    dims = oracle.dims_for("tiny")
    sd = oracle.synthetic_state_dict(dims, seed=11)
    om = oracle.OracleModel(dims, sd, sdpa=True)
    tok = get_tokenizer(True, num_languages=dims.n_vocab - 51765 - 1, language="en", task="transcribe")
    init = list(tok.sot_sequence)
    suppress = sorted(set(list(tok.non_speech_tokens) + [tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm,
                                                         tok.no_speech, tok.eot]))
    rules = oracle.SamplingRules(sample_begin=len(init), sot_index=0, eot=tok.eot, n_ctx=dims.n_text_ctx,
                                 timestamp_begin=tok.timestamp_begin, no_timestamps=tok.no_timestamps, suppress_tokens=suppress,
                                 blank_token=tok.encode(" ")[0], no_speech=tok.no_speech)
    g = torch.Generator().manual_seed(12)
    feats = (torch.randn(ROWS_MAX, dims.n_audio_ctx, dims.n_audio_state, generator=g)
             + 3.0 * torch.randn(ROWS_MAX, 1, dims.n_audio_state, generator=g)).half().float()
    condition.condition_greedy(om, feats, init, N_STEPS, rules, seed=5, margin=(0.35, 3.0), text_run=(4, 14), passes=2)
    mask = torch.zeros(dims.n_vocab, dtype=torch.uint8)
    mask[suppress] = 1
    mask = mask.to(gpu_device)
    params = hip.GreedyParams(sample_begin=len(init), max_steps=N_STEPS, n_ctx=dims.n_text_ctx, eot=tok.eot,
                              timestamp_begin=tok.timestamp_begin, no_timestamps=tok.no_timestamps,
                              max_initial_timestamp_index=50, suppress_blank=1, blank_token=tok.encode(" ")[0],
                              suppress_mask=mask.data_ptr())
    model = hip.HipModel(dims, hip.WH_F16, hip.pack_weights(om.sd, dims, hip.WH_F16, gpu_device))
    return {"dims": dims, "om": om, "init": init, "rules": rules, "params": params, "mask": mask, "feats": feats, "tok": tok,
            "model": model}


@pytest.mark.parametrize("R", [17, 24])
def test_step_ln_post_equals_ln_prologue(conditioned, gpu_device, R):
    c = conditioned
    model, init, T0 = c["model"], c["init"], len(c["init"])
    feats = c["feats"][:R]
    with torch.no_grad():
        want = oracle.greedy_decode(c["om"], feats, init, N_STEPS, c["rules"], keep_logits=True)
    mg = condition.margins_of(want)
    assert mg["min"] >= 0.3 and mg.get("rule_min", 1.0) >= 0.3, mg      # rows are independent: the margins built at 24 rows hold
    path = want["tokens"].to(gpu_device)
    dfeats = feats.to(gpu_device).half().contiguous()

    def run(flags, want_sites):
        task = hip.HipTask(model, R, 1, 8, extra_flags=flags)
        try:
            tokens = torch.zeros(R, T0 + N_STEPS + 1, dtype=torch.int64, device=gpu_device)
            tokens[:, :T0] = torch.tensor(init, device=gpu_device)
            task.reset()
            task.set_audio(dfeats)
            n, _, _ = task.greedy(tokens, c["params"], 0, c["tok"].no_speech)
            assert n == T0 + N_STEPS and task.ln_post_sites == want_sites
            ids = tokens[:, :n].cpu()
            task.reset()
            task.set_audio(dfeats)
            logits = [task.prefill(path[:, :T0].contiguous())[:, -1].float().cpu()]
            for i in range(N_STEPS - 1):
                logits.append(task.step(path[:, T0 + i]).float().cpu())
            return ids, torch.stack(logits)
        finally:
            task.close()
            model.drop_cached_tasks()

    ids_old, old = run(hip.WH_TASK_LN_PROLOGUE, 0)
    ids_new, new = run(0, 2)
    assert torch.isfinite(old).all() and torch.isfinite(new).all()
    assert torch.equal(old[0], new[0])                                 # the prefill
    d = (new - old).abs().max().item()
    print(f"rows {R}: max |dlogit| {d:.4g} over {N_STEPS} steps; oracle margins {mg}")
    assert torch.equal(ids_new, ids_old), "token ids differ between the two forms"
    assert torch.equal(ids_new, want["tokens"]), "token ids differ from the oracle's"
    assert d <= 6e-2, d
