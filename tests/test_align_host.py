"""Duration control and the forced aligner, host side (CPU only): the numpy textbook Monotonic Alignment Search that is
the specification of mt_align, the condition under which the GPU recovery test means something (the textbook search
recovers planted durations, the trainer's reference recurrence does not), and synthesize's argument errors.

The helpers here (textbook_mas, planted, log_prior_*) are shared with tests/test_gpu_align.py and
tests/test_gpu_durations.py."""
import math

import numpy as np
import pytest
import torch

from conftest import make_matcha

NEG = np.float32(-1e9)


def textbook_mas(lp: np.ndarray, tx: int, ty: int):
    """Glow-TTS / upstream Matcha `maximum_path_each` on one utterance's log-prior lp [Tx][Ty] (any float dtype; the
    arithmetic is lp's): -> (durations int64 [Tx], path float32 [Tx][Ty]). Cells max(0, tx+y-ty) <= x < min(tx, y+1):
    p[x][y] = lp[x][y] + max(cur, prev), cur = NEG if x == y else p[x][y-1],
    prev = (0 if y == 0 else NEG) if x == 0 else p[x-1][y-1]; then the backtrack from (tx-1, ty-1)."""
    Tx, Ty = lp.shape
    dur = np.zeros(Tx, dtype=np.int64)
    path = np.zeros((Tx, Ty), dtype=np.float32)
    tx, ty = min(max(tx, 0), Tx), min(max(ty, 0), Ty)
    if tx <= 0 or ty < tx:
        return dur, path
    neg = lp.dtype.type(-1e9)
    p = lp.copy()
    for y in range(ty):
        lo, hi = max(0, tx + y - ty), min(tx, y + 1)
        xs = np.arange(lo, hi)
        cur = np.where(xs == y, neg, p[xs, y - 1] if y > 0 else neg)
        prev = np.where(xs == 0, lp.dtype.type(0) if y == 0 else neg, p[xs - 1, y - 1] if y > 0 else neg)
        p[xs, y] = lp[xs, y] + np.maximum(cur, prev)
    idx = tx - 1
    for y in range(ty - 1, -1, -1):
        dur[idx] += 1
        path[idx, y] = 1.0
        if idx != 0 and (idx == y or p[idx, y - 1] < p[idx - 1, y - 1]):
            idx -= 1
    return dur, path


def textbook_mas_serial(lp: np.ndarray, tx: int, ty: int):
    """the same recurrence one cell at a time, x ascending (the serial loop the vectorised form must equal)"""
    p = lp.copy()
    neg = lp.dtype.type(-1e9)
    for y in range(ty):
        for x in range(max(0, tx + y - ty), min(tx, y + 1)):
            cur = neg if x == y else p[x, y - 1]
            prev = (lp.dtype.type(0) if y == 0 else neg) if x == 0 else (p[x - 1, y - 1] if y > 0 else neg)
            p[x, y] = lp[x, y] + max(cur, prev)
    dur = np.zeros(lp.shape[0], dtype=np.int64)
    idx = tx - 1
    for y in range(ty - 1, -1, -1):
        dur[idx] += 1
        if idx != 0 and (idx == y or p[idx, y - 1] < p[idx - 1, y - 1]):
            idx -= 1
    return dur


def planted(seed=7, B=3, Tx=37, x_lengths=(37, 20, 1), noise=0.05, C=80, mu=None):
    """mu [B,C,Tx] (random, or the one given), known durations 1..6 per token (0 past x_lengths), and
    mel = mu expanded by them + N(0, noise^2) -> (mu, mel [B,C,Ty], durations int64 [B,Tx], y_lengths int64 [B])."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(1, 7, (B, Tx), generator=g)
    xl = torch.tensor(x_lengths)
    d = d * (torch.arange(Tx)[None] < xl[:, None])
    if mu is None:
        mu = torch.randn(B, C, Tx, generator=g)
    yl = d.sum(1)
    Ty = int(yl.max())
    mel = torch.zeros(B, mu.shape[1], Ty)
    for b in range(B):
        mel[b, :, :int(yl[b])] = torch.repeat_interleave(mu[b], d[b], dim=1)
    mel = mel + noise * torch.randn(mel.shape, generator=g)
    return mu, mel, d, yl


def log_prior_direct(mu, y, dtype=torch.float64):
    """-0.5 sum_c (y[c][j] - mu[c][x])^2 - 0.5 C log(2 pi) in `dtype` -> [B,Tx,Ty]"""
    mu, y = mu.to(dtype), y.to(dtype)
    d = y[:, :, None, :] - mu[:, :, :, None]
    return -0.5 * (d * d).sum(1) - 0.5 * mu.shape[1] * math.log(2 * math.pi)


def log_prior_expanded(mu_x, y):
    """the reference's expanded expression as the oracle states it (oracle/matcha_oracle.py training_losses,
    train_standalone.py:639-644), in the inputs' dtype"""
    const = -0.5 * math.log(2 * math.pi) * mu_x.shape[1]
    factor = -0.5 * torch.ones(mu_x.shape, dtype=mu_x.dtype)
    y_square = torch.matmul(factor.transpose(1, 2), y ** 2)
    y_mu_double = torch.matmul(2.0 * (factor * mu_x).transpose(1, 2), y)
    mu_square = torch.sum(factor * (mu_x ** 2), 1).unsqueeze(-1)
    return y_square - y_mu_double + mu_square + const


def reference_mas_durations(lp, xl, yl):
    """frames per token under the trainer's reference recurrence (oracle.maximum_path)"""
    from oracle import matcha_oracle as O
    B, Tx, Ty = lp.shape
    mask = (O.sequence_mask(xl, Tx)[:, :, None] & O.sequence_mask(yl, Ty)[:, None, :]).float()
    return O.maximum_path(lp, mask).sum(-1).long()


@pytest.mark.parametrize("noise", [0.05, 0.5])
def test_textbook_mas_recovers_planted_durations_and_the_reference_recurrence_does_not(noise):
    mu, mel, d, yl = planted(noise=noise)
    xl = torch.tensor([37, 20, 1])
    lp64 = log_prior_direct(mu, mel)
    lp32 = log_prior_direct(mu, mel, torch.float32)
    assert lp32.dtype == torch.float32
    for lp in (lp64, lp32):
        for b in range(3):
            dur, path = textbook_mas(lp[b].numpy(), int(xl[b]), int(yl[b]))
            assert np.array_equal(dur, d[b].numpy()), (noise, b)
            assert np.array_equal(path.sum(1), d[b].numpy()) and path[:, :int(yl[b])].sum(0).min() == 1
    ref = reference_mas_durations(lp32, xl, yl)
    # the reference recurrence piles the frames on one early token: rows like [5, 88, 1, 1, 1, ...]
    for b in (0, 1):
        assert not torch.equal(ref[b], d[b])
        assert (ref[b] - d[b]).abs().sum() > 2 * int(xl[b]) and ref[b].max() > 40


def test_vectorised_specification_equals_the_serial_loop():
    mu, mel, d, yl = planted(seed=3, B=2, Tx=11, x_lengths=(11, 4), noise=2.0)
    lp = log_prior_direct(mu, mel, torch.float32).numpy()
    for b, tx in enumerate((11, 4)):
        for ty in (int(yl[b]), tx, tx + 1):
            assert np.array_equal(textbook_mas(lp[b], tx, ty)[0], textbook_mas_serial(lp[b], tx, ty))
    assert textbook_mas(lp[0], 11, 11)[0].tolist() == [1] * 11
    assert textbook_mas(lp[0], 1, 9)[0].tolist() == [9] + [0] * 10
    assert textbook_mas(lp[0], 5, 4)[0].sum() == 0 and textbook_mas(lp[0], 0, 4)[0].sum() == 0


def test_direct_and_expanded_log_prior_are_one_function():
    mu, mel, _, _ = planted()
    a, b = log_prior_direct(mu, mel), log_prior_expanded(mu.double(), mel.double())
    assert (a - b).abs().max() < 1e-11
    e32 = (log_prior_expanded(mu, mel).double() - a).abs().max().item()
    print(f"expanded fp32 vs fp64: {e32:.3e}")
    assert 1e-6 < e32 < 1e-3


def test_duration_arguments_raise_without_a_gpu():
    m = make_matcha(1)
    x, xl = torch.randint(1, 178, (2, 9)), torch.tensor([9, 6])
    d = torch.ones(2, 9, dtype=torch.int64)
    with pytest.raises(ValueError, match="length_scale"):
        m.synthesize(x, xl, 2, durations=d, length_scale=1.2)
    with pytest.raises(ValueError, match="length_scale"):
        m.synthesize(x, xl, 2, durations=d, length_scale=torch.ones(2))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, 2, durations=d, token_scale=torch.ones(2, 9))
    with pytest.raises(ValueError, match=r"\(2, 9\)"):
        m.synthesize(x, xl, 2, durations=d[:, :8])
    with pytest.raises(ValueError, match=r"\(2, 9\)"):
        m.synthesize(x, xl, 2, token_scale=[[1.0] * 9])
    with pytest.raises(TypeError):
        m.synthesize(x, xl, 2, durations=d.float())
    with pytest.raises(ValueError):
        m.synthesise(x, xl, 2, durations=d, length_scale=0.9)
    with pytest.raises(ValueError):
        m.predict_durations(x, xl, token_scale=torch.ones(9))


def test_duration_args_pass_through():
    from matcha_hip import runtime as rt
    assert rt.duration_args(2, 3) == (None, None)
    assert rt.duration_args(2, 3, length_scale=[1.0, 2.0]) == (None, None)
    ts, d = rt.duration_args(2, 3, token_scale=[[1, 2, 3], [0.5, 1, 1]])
    assert d is None and ts.dtype == torch.float32 and ts.shape == (2, 3)
    ts, d = rt.duration_args(2, 3, durations=[[1, 0, 3], [2, 2, 0]])
    assert ts is None and d.dtype == torch.float32 and d.tolist() == [[1, 0, 3], [2, 2, 0]]
