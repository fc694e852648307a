"""The stock logit rules of whisper_amd/csrc/logit_rules.h on the host: `rule_masked` over every token of a row, through
wht_rule_mask (ktest.cpp; nothing is launched), against the -inf positions that oracle.decoding.apply_filters leaves on an
all-finite row — for EVERY history of 0 to 3 sampled tokens over a token set that holds one of each kind the rules tell
apart, on a vocabulary of 40.  The "timestamp mass" rule is not an entry's own and stays out (mass_rule=False).

The sampler and the beam update reach the row's timestamp window in two ways: from the row's tokens (beam.hip; the host
entry follows the same definition) and from the three words of row_state that greedy_final_kernel keeps per row
(sampling.hip).  Both must give the same window for every history: that is what lets the sampler do without the scan.
"""
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_lib  # noqa: E402
from oracle.decoding import SamplingRules, apply_filters  # noqa: E402

V, EOT, TB, NO_TS, BLANK = 40, 20, 24, 23, 3
SUPPRESS = (5, 21, 30)
TOKENS = (7, EOT - 1, TB, 27, 33, V - 1)        # a text token, eot - 1, timestamp_begin, two later timestamps, V - 1
T0 = 3                                          # sample_begin of the longest row
HISTORIES = [h for n in range(4) for h in itertools.product(TOKENS, repeat=n)]


def state_after(history, tb):
    """row_state words 0..2 as greedy_final_kernel leaves them (sampling.hip, `if (ts_rules)` behind the token's store), from
    all-zero: [1] <- [0]; [0] <- the token is a timestamp; [2] <- the token + 1 if it is"""
    st = [0, 0, 0]
    for tok in history:
        st[1] = st[0]
        st[0] = int(tok >= tb)
        if tok >= tb:
            st[2] = tok + 1
    return st


def device_rules(history, lag, tb, max_initial, suppress_blank, mask, row_state=None):
    """-> (mask [V] bool, window (last_ts, pen_ts, lo, hi)) of logit_rules.h for a row of T0 - lag prompt tokens + history"""
    row = np.array([1] * (T0 - lag) + list(history), dtype=np.int64)
    out, window = np.full(V, 7, np.uint8), np.full(4, -9, np.int32)
    rs = np.array(row_state, np.int32) if row_state is not None else None
    kernel_lib.lib().wht_rule_mask(row.ctypes.data, T0 + len(history), lag, V, T0, EOT, tb, NO_TS, max_initial, suppress_blank, BLANK,
                                   mask.ctypes.data, rs.ctypes.data if rs is not None else None, out.ctypes.data,
                                   window.ctypes.data)
    assert set(out.tolist()) <= {0, 1}
    return out.astype(bool), tuple(window.tolist())


def test_mask_equals_the_filters_on_every_short_history():
    mask = np.zeros(V, np.uint8)
    mask[list(SUPPRESS)] = 1
    rows = 0
    for with_ts, max_initial, suppress_blank in itertools.product((True, False), (-1, 0, 5), (1, 0)):
        r = SamplingRules(sample_begin=T0, sot_index=0, eot=EOT, n_ctx=448, timestamp_begin=TB if with_ts else None,
                          no_timestamps=NO_TS, max_initial_timestamp_index=None if max_initial < 0 else max_initial,
                          suppress_blank=bool(suppress_blank), blank_token=BLANK, suppress_tokens=list(SUPPRESS))
        tb = TB if with_ts else -1
        for H in HISTORIES:
            x = torch.zeros(V)
            apply_filters(x, list(H), r, mass_rule=False)
            want = (x == -np.inf).numpy()
            assert np.isfinite(x.numpy()[~want]).all()
            for lag in (0, 2):
                got, window = device_rules(H, lag, tb, max_initial, suppress_blank, mask)
                assert np.array_equal(got, want), (with_ts, max_initial, suppress_blank, H, lag, np.flatnonzero(got != want))
                # the greedy loop's state gives the same window, hence the same mask
                got_s, window_s = device_rules(H, lag, tb, max_initial, suppress_blank, mask, row_state=state_after(H, TB))
                assert window_s == window, (with_ts, H, lag, window_s, window)
                assert np.array_equal(got_s, want)
                if not with_ts:
                    assert window == (0, 0, 0, 0)
                rows += 1
    assert rows == 2 * 3 * 2 * 259 * 2

