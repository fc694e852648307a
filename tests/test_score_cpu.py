"""Teacher-forced scoring without a GPU: the float64 restatement on a hand-computed case, the argument statuses of the two
new C calls, and the refusals `whisper_amd.score` raises before any device work."""
import ctypes
import math

import pytest
import torch

import score_oracle
import whisper_amd
from whisper_amd import hip


def test_restatement_on_a_hand_computed_case():
    """3 x 5 logits built from logarithms, so every log-sum is the logarithm of a small integer:
         row 0: log 1, log 2, log 3, log 4, log 6      row 1: log 2, log 5, log 5, log 1, log 9      row 2: a padded slot"""
    L = torch.log(torch.tensor([[1., 2., 3., 4., 6.], [2., 5., 5., 1., 9.], [7., 1., 1., 1., 1.]], dtype=torch.float64))
    # all five columns: sums 16 and 22
    lp, tl, tt = score_oracle.score_rows(L, torch.tensor([2, 4, -1]), 5)
    assert lp.tolist() == pytest.approx([math.log(3 / 16), math.log(9 / 22), 0.0], abs=1e-15)
    assert tl.tolist() == pytest.approx([math.log(6 / 16), math.log(9 / 22), 0.0], abs=1e-15)
    assert tt.tolist() == [4, 4, -1]
    # v_end = 3 cuts the sums to 6 and 12; row 1's maximum 5 is attained twice: the lowest id wins
    lp, tl, tt = score_oracle.score_rows(L, torch.tensor([0, 2, -1]), 3)
    assert lp.tolist() == pytest.approx([math.log(1 / 6), math.log(5 / 12), 0.0], abs=1e-15)
    assert tl.tolist() == pytest.approx([math.log(3 / 6), math.log(5 / 12), 0.0], abs=1e-15)
    assert tt.tolist() == [2, 1, -1]
    # a target at v_end and one beyond it: -inf, the top entries unaffected
    lp, tl, tt = score_oracle.score_rows(L, torch.tensor([3, 4, 0]), 3)
    assert lp[0] == -math.inf and lp[1] == -math.inf
    assert lp[2].item() == pytest.approx(math.log(7 / 9), abs=1e-15)
    assert tt.tolist() == [2, 1, 0]
    # v_end = 1: one column, probability one
    lp, tl, tt = score_oracle.score_rows(L, torch.tensor([0, 0, -1]), 1)
    assert lp.tolist() == [0.0, 0.0, 0.0] and tl.tolist() == [0.0, 0.0, 0.0] and tt.tolist() == [0, 0, -1]


def test_null_arguments_of_the_c_calls():
    lib = hip.lib()
    assert lib.wh_score_scratch_bytes(None, 4, 16) == 0
    n_tok = (ctypes.c_int32 * 1)(2)
    assert lib.wh_task_score(None, None, 0, 2, n_tok, 0, 1, None, None, None, None, 0, None) == 1     # WH_ERR_ARG
    assert lib.wh_status_string(1) == b"invalid argument"


class _NoDeviceModel:
    """what `score` reads before it touches the device"""
    is_multilingual, num_languages = True, 99


def test_refusals_before_any_device_work():
    from whisper_amd.synthetic import dims_for
    model = _NoDeviceModel()
    model.dims = dims_for("tiny")
    mel = torch.zeros(2, 80, 3000)
    opts = whisper_amd.DecodingOptions(language="en", fp16=False)
    with pytest.raises(ValueError, match="vocabulary"):
        whisper_amd.score(model, mel, [[[1]], [[2]]], opts, vocabulary="speech")
    with pytest.raises(ValueError, match="hypothesis lists"):
        whisper_amd.score(model, mel, [[[1]]], opts)
    with pytest.raises(ValueError, match="prompts"):
        whisper_amd.score(model, mel, [[[1]], [[2]]], opts, prompts=[[5]])
    too_long = [7] * (model.dims.n_text_ctx - 3)            # + 3 sot tokens + <|endoftext|> = n_text_ctx + 1
    with pytest.raises(ValueError, match="n_text_ctx"):
        whisper_amd.score(model, mel, [[[1]], [too_long]], opts)
    with pytest.raises(ValueError, match="vocabulary"):
        whisper_amd.score(model, mel, [[[1]], [[model.dims.n_vocab]]], opts)


def test_score_result_is_frozen_and_exported():
    r = whisper_amd.ScoreResult(tokens=[1], token_logprobs=[-1.0, -2.0], sum_logprob=-3.0, avg_logprob=-1.5,
                                top_tokens=[1, 2], top_logprobs=[-1.0, -0.5], language="en")
    with pytest.raises(Exception):
        r.sum_logprob = 0.0
    assert whisper_amd.score is whisper_amd.decoding.score
