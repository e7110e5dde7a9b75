"""The forced aligner mt_align (MI355X): the direct-form log-prior against fp64, the search against the numpy textbook
MAS of tests/test_align_host.py run on the device's own log-prior, recovery of planted durations (which the trainer's
reference recurrence does not achieve), independence from the batch, and prosody transfer end to end."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import make_matcha
from test_align_host import log_prior_expanded, planted, textbook_mas

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _random_case(B, Tx, Ty, seed):
    """mu ~ N(0, 1) and a normalized mel ~ N(0.2, 1.3^2): |log-prior| ~ 180; and a denormalized copy of the mel
    with per-channel statistics around LJSpeech's"""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, 80, Tx, generator=g)
    yn = 1.3 * torch.randn(B, 80, Ty, generator=g) + 0.2
    mean = -5.536 + 0.3 * torch.randn(80, generator=g)
    std = 2.116 * (1 + 0.1 * torch.rand(80, generator=g))
    mel = yn * std[None, :, None] + mean[None, :, None]
    return mu, yn, mel, mean, std


def _lp64(mu, yh64):
    d = yh64[:, :, None, :] - mu.double()[:, :, :, None]
    return -0.5 * (d * d).sum(1) - 0.5 * mu.shape[1] * math.log(2 * math.pi)


# ---------------------------------------------------------------- 1. the log-prior
@pytest.mark.parametrize("norm", [False, True], ids=["normalized", "mean-std"])
@pytest.mark.parametrize("B,Tx,Ty", [(3, 37, 140), (1, 300, 320)])
def test_log_prior_is_no_worse_than_the_expanded_form(B, Tx, Ty, norm):
    """max |lp - fp64| of the device's direct form must not exceed that of the oracle's fp32 expanded expression
    (train_standalone.py:639-644) on the same inputs. Measured on the MI355X: 1.5e-5 to 2.2e-5 against 4.7e-5 to
    5.1e-5."""
    from matcha_hip import runtime as rt
    mu, yn, mel, mean, std = _random_case(B, Tx, Ty, seed=Tx)
    lens = (torch.full((B,), Tx), torch.full((B,), Ty))
    if norm:
        truth = _lp64(mu, (mel.double() - mean.double()[None, :, None]) / std.double()[None, :, None])
        oracle = log_prior_expanded(mu, (mel - mean[None, :, None]) / std[None, :, None])
        _, _, lp = rt.align(mu.to(DEV), mel.to(DEV), *lens, mean=mean, std=std, want_log_prior=True)
    else:
        truth = _lp64(mu, yn.double())
        oracle = log_prior_expanded(mu, yn)
        _, _, lp = rt.align(mu.to(DEV), yn.to(DEV), *lens, want_log_prior=True)
    assert oracle.dtype == torch.float32 and lp.dtype == torch.float32 and lp.shape == (B, Tx, Ty)
    e_gpu = (lp.cpu().double() - truth).abs().max().item()
    e_ref = (oracle.double() - truth).abs().max().item()
    print(f"B={B} Tx={Tx} Ty={Ty} norm={norm}: |lp| ~ {truth.abs().mean():.0f}, device max|d| {e_gpu:.3e}, "
          f"expanded fp32 max|d| {e_ref:.3e}")
    assert e_gpu <= e_ref, (e_gpu, e_ref)


# ---------------------------------------------------------------- 2. the search
MAS_CASES = {
    # t_xs, t_ys per row: full / ty == tx (all ones) / tx == 1
    "3x37x140": (37, 140, [37, 20, 1], [140, 20, 77]),
    "1x300x320": (300, 320, [300], [320]),
    # sixteen waves, and lengths to clamp or refuse: ty < tx, no tokens, lengths past the table
    "1x1024x1100": (1024, 1100, [1000], [1100]),
    "4x9x40": (9, 40, [5, 0, 12, 9], [3, 10, 2000, 9]),
}


@pytest.mark.parametrize("case", list(MAS_CASES))
def test_search_equals_the_textbook_specification(case):
    from matcha_hip import runtime as rt
    Tx, Ty, t_xs, t_ys = MAS_CASES[case]
    B = len(t_xs)
    mu, yn, _, _, _ = _random_case(B, Tx, Ty, seed=Ty)
    dur, attn, lp = rt.align(mu.to(DEV), yn.to(DEV), t_xs, t_ys, want_attn=True, want_log_prior=True)
    assert dur.dtype == torch.int64 and dur.shape == (B, Tx) and attn.shape == (B, Tx, Ty)
    lp_h = lp.cpu().numpy()
    for b in range(B):
        d_spec, p_spec = textbook_mas(lp_h[b], t_xs[b], t_ys[b])
        assert np.array_equal(dur[b].cpu().numpy(), d_spec), (case, b)
        assert np.array_equal(attn[b].cpu().numpy(), p_spec), (case, b)
        tx, ty = min(max(t_xs[b], 0), Tx), min(max(t_ys[b], 0), Ty)
        assert int(dur[b].sum()) == (ty if 0 < tx <= ty else 0)
        assert int(dur[b, tx:].sum()) == 0
        if tx == ty:
            assert dur[b, :tx].tolist() == [1] * tx
    # durations alone (no attn, no log-prior kept) are the same
    assert torch.equal(rt.align(mu.to(DEV), yn.to(DEV), t_xs, t_ys)[0], dur)


# ---------------------------------------------------------------- 3. recovery
@functools.lru_cache(maxsize=None)
def _matcha():
    from matcha_hip import synthetic
    m = make_matcha(1, "fp32")
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in m.state_dict().items()], 5).items()}
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _reference_recurrence(lp, xl, yl):
    """frames per token under the trainer's recurrence, on the device (rt.maximum_path)"""
    from matcha_hip import runtime as rt
    B, Tx, Ty = lp.shape
    mask = ((torch.arange(Tx)[None] < xl[:, None])[:, :, None] & (torch.arange(Ty)[None] < yl[:, None])[:, None, :])
    return rt.maximum_path(lp, mask.float().to(DEV)).sum(-1).long().cpu()


def test_recovers_planted_durations_where_the_reference_recurrence_does_not():
    from matcha_hip import runtime as rt
    xl = torch.tensor([37, 20, 1])
    mu, mel, d, yl = planted()
    dur, _, lp = rt.align(mu.to(DEV), mel.to(DEV), xl, yl, want_log_prior=True)
    assert torch.equal(dur.cpu(), d)
    ref = _reference_recurrence(lp, xl, yl)
    for b in (0, 1):
        assert (ref[b] - d[b]).abs().sum() > 2 * int(xl[b]), ref[b].tolist()


def test_model_align_recovers_planted_durations():
    """the same through MatchaTTS.align: the encoder's mu on synthetic weights, the mel denormalized as synthesize
    returns it"""
    from matcha_hip import runtime as rt
    m = _matcha()
    xl = torch.tensor([37, 20, 1])
    x = torch.randint(1, 178, (3, 37), generator=torch.Generator().manual_seed(37))
    mu, _, _ = m.encoder(x.to(DEV), xl.to(DEV))
    _, mel_n, d, yl = planted(mu=mu.cpu())
    mel = mel_n * m.mel_std.cpu() + m.mel_mean.cpu()
    dur, attn = m.align(x.to(DEV), xl.to(DEV), mel.to(DEV), yl, return_attn=True)
    print(f"spread of neighbouring mu columns: {(mu[0, :, 1:] - mu[0, :, :-1]).norm(dim=0).min().item():.2f}")
    assert torch.equal(dur.cpu(), d)
    assert attn.shape == (3, 1, 37, mel.shape[-1]) and torch.equal(attn[:, 0].sum(-1).long().cpu(), d)
    assert torch.equal(m.align(x.to(DEV), xl.to(DEV), mel_n.to(DEV), yl.to(DEV), normalized=True).cpu(), d)
    _, _, lp = rt.align(mu, mel_n.to(DEV), xl, yl, want_log_prior=True)
    ref = _reference_recurrence(lp, xl, yl)
    for b in (0, 1):
        assert (ref[b] - d[b]).abs().sum() > 2 * int(xl[b]), ref[b].tolist()
    with pytest.raises(ValueError):
        m.align(x.to(DEV), xl.to(DEV), mel.to(DEV), torch.tensor([int(yl[0]), 19, 5]))


# ---------------------------------------------------------------- 4. independence from the batch
def test_a_row_does_not_depend_on_its_batch():
    from matcha_hip import runtime as rt
    mu, yn, mel, mean, std = _random_case(3, 70, 200, seed=70)
    t_xs, t_ys = [70, 33, 64], [200, 129, 65]
    for kw, y in ((dict(), yn), (dict(mean=mean, std=std), mel)):
        dur, _, lp = rt.align(mu.to(DEV), y.to(DEV), t_xs, t_ys, want_log_prior=True, **kw)
        for b, (tx, ty) in enumerate(zip(t_xs, t_ys)):
            d1, _, lp1 = rt.align(mu[b:b + 1, :, :tx].to(DEV), y[b:b + 1, :, :ty].to(DEV), [tx], [ty],
                                  want_log_prior=True, **kw)
            assert torch.equal(lp1[0], lp[b, :tx, :ty]), b
            assert torch.equal(d1[0], dur[b, :tx]) and int(dur[b, tx:].sum()) == 0


# ---------------------------------------------------------------- 5. prosody transfer
def test_prosody_transfer_end_to_end():
    m = _matcha()
    g = torch.Generator().manual_seed(5)
    x, xl = torch.randint(1, 178, (3, 24), generator=g).to(DEV), torch.tensor([24, 17, 9], device=DEV)
    d0 = torch.randint(1, 6, (3, 24), generator=g) * (torch.arange(24)[None] < xl.cpu()[:, None])
    seeds = [1, 2, 3]
    mel, yl, _ = m.synthesize(x, xl, 2, seeds=seeds, durations=d0)
    assert torch.equal(yl.cpu(), d0.sum(1))
    d1 = m.align(x, xl, mel, yl)
    assert d1.shape == (3, 24) and torch.equal(d1.sum(1), yl) and int(d1[1, 17:].sum()) == 0
    print(f"tokens whose duration the aligner gives back: {int((d1.cpu() == d0).sum())} of {int(xl.sum())}")
    mel2, yl2, _ = m.synthesize(x, xl, 2, seeds=seeds, durations=d1)
    assert torch.equal(yl2, yl) and mel2.shape == mel.shape
