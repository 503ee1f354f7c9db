"""Windows of a time series for sequence models (src/data/sequences.jl: split_into_sequences, filter_sequences).

The engine never materialises windows: a window is its start row in the series that lives in HBM (HybridEngine.set_sequences), and
with output_shift = 1 neighbouring windows share all but one row.  The (feature, time, batch) arrays the reference builds are returned
as well, for inspection and for tests.

0-based, W = input_window, ow = output_window, s = output_shift, lam = lead_time, series of L rows:
starts a = 0, s, 2s, ... <= L - W - lam; inputs (and forcings) of a window are rows a .. a + W - 1; prediction j < ow is the model's
output at input step W - ow + j and is compared with the target at row a + W - ow + j + lam (sequences.jl:203-229,
compute_loss.jl:104-110).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Sequences(NamedTuple):
    starts: np.ndarray          # (n_windows,) int32: first row of every window
    x: np.ndarray               # (feature, input_window, n_windows) float32
    y: np.ndarray               # (target, output_window, n_windows) float32
    input_window: int
    output_window: int
    lead_time: int

    def target_rows(self, w: int = None) -> np.ndarray:
        """rows of the series the ow predictions of window w are compared with ((n_windows, ow) for all windows)"""
        off = self.input_window - self.output_window + self.lead_time + np.arange(self.output_window)
        return (self.starts[:, None] + off[None, :]) if w is None else self.starts[w] + off


def split_into_sequences(x, y, *, input_window: int = 5, output_window: int = 1, output_shift: int = 1, lead_time: int = 1) -> Sequences:
    """x (feature, time), y (target, time) -> the window starts and the materialised windows (sequences.jl:188-241)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if x.ndim != 2:
        raise ValueError(f"expected x to be (feature, time); got ndims(x) = {x.ndim}")
    if y.ndim != 2:
        raise ValueError(f"expected y to be (target, time); got ndims(y) = {y.ndim}")
    L = x.shape[1]
    if y.shape[1] != L:
        raise ValueError(f"x and y must have same time length; got {L} vs {y.shape[1]}")
    if lead_time < 0:
        raise ValueError("lead_time must be ≥ 0 (0 = instantaneous end)")
    if not 1 <= output_window <= input_window:
        raise ValueError(f"output_window must be 1..input_window; got {output_window} with input_window {input_window}")
    if output_shift < 1:
        raise ValueError(f"output_shift must be ≥ 1; got {output_shift}")
    last = L - input_window - lead_time
    if last < 0:
        raise ValueError("windows too long for series length")
    starts = np.arange(0, last + 1, output_shift, dtype=np.int32)
    rows_x = starts[None, :] + np.arange(input_window)[:, None]                                       # (W, n)
    rows_y = starts[None, :] + (input_window - output_window + lead_time) + np.arange(output_window)[:, None]      # (ow, n)
    return Sequences(starts, x[:, rows_x], y[:, rows_y], int(input_window), int(output_window), int(lead_time))


def filter_sequences(seq: Sequences) -> Sequences:
    """drop the windows with a NaN predictor in their input rows, or whose target values are all NaN (sequences.jl: filter_sequences)"""
    bad_x = np.isnan(seq.x).any(axis=(0, 1))
    bad_y = np.isnan(seq.y).all(axis=(0, 1))
    keep = ~(bad_x | bad_y)
    return Sequences(seq.starts[keep], seq.x[:, :, keep], seq.y[:, :, keep], seq.input_window, seq.output_window, seq.lead_time)
