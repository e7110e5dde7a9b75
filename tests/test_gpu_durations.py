"""Duration control (MI355X): mt_durations_tokens at the op level (per-token scale, given durations, the `bad` flag),
synthesize(durations=predict_durations(...)) as a bit-exact round trip in both estimator precisions, and edited
durations end to end against the oracle."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import HP, make_matcha

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(B, Tx, seed):
    g = torch.Generator().manual_seed(seed)
    logw = torch.randn(B, 1, Tx, generator=g) * 0.7 + 0.6
    lens = torch.tensor([Tx, max(1, (2 * Tx) // 3), max(1, Tx // 4)][:B])
    x_mask = (torch.arange(Tx)[None] < lens[:, None]).float()[:, None]
    ls = torch.tensor([0.8, 1.0, 1.25][:B])
    ts = torch.rand(B, Tx, generator=g) * 1.5 + 0.5
    return logw, x_mask, ls, ts


def _near_integer(v64: np.ndarray) -> np.ndarray:
    """the fp64 value lies within one fp32 ulp of a whole number: there the ceil may go either way"""
    return np.abs(v64 - np.round(v64)) <= np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------- 1. the op
@pytest.mark.parametrize("B,Tx", [(1, 1), (3, 37), (2, 300)])
def test_token_scale_of_ones_is_the_per_utterance_call(B, Tx):
    from matcha_hip import runtime as rt
    logw, x_mask, ls, _ = _inputs(B, Tx, seed=Tx)
    a = rt.durations(logw.to(DEV), x_mask.to(DEV), ls)
    b = rt.durations(logw.to(DEV), x_mask.to(DEV), ls, token_scale=torch.ones(B, Tx))
    assert len(a) == 3 and len(b) == 4
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert b[3].dtype == torch.int32 and b[3].item() == 0
    # no length scale at all: the scalar call's bits
    c = rt.durations(logw.to(DEV), x_mask.to(DEV), 1.0, token_scale=torch.ones(B, Tx, device=DEV))
    for u, v in zip(rt.durations(logw.to(DEV), x_mask.to(DEV), 1.0), c):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B,Tx", [(1, 1), (3, 37), (2, 300)])
def test_token_scale_matches_torch(B, Tx):
    """ceil(((exp(logw) * m) * ls) * ts) in torch fp32 on the CPU. The device's exp may differ from the host's in
    the last bit, which flips a ceil only where the value sits on a whole number: a differing token must lie within
    one fp32 ulp of one in fp64, and at most 1 % may. The seeds are ones for which the host's own fp32 result equals
    the fp64 one at every token."""
    from matcha_hip import runtime as rt
    logw, x_mask, ls, ts = _inputs(B, Tx, seed=Tx)
    want = torch.ceil(((torch.exp(logw) * x_mask) * ls[:, None, None]) * ts[:, None])
    v64 = (np.exp(logw.double().numpy()) * x_mask.double().numpy() * ls.double().numpy()[:, None, None]
           * ts.double().numpy()[:, None])
    assert np.array_equal(np.ceil(v64), want.numpy().astype(np.float64)), "seed: the host fp32 / fp64 results differ"
    w_ceil, cum, yl, bad = rt.durations(logw.to(DEV), x_mask.to(DEV), ls, token_scale=ts)
    got = w_ceil.cpu()
    diff = (got != want).numpy()
    print(f"B={B} Tx={Tx}: {int(diff.sum())} of {diff.size} tokens differ from the host")
    assert diff.sum() <= 0.01 * diff.size
    assert _near_integer(v64)[diff].all()
    assert np.abs(got.numpy() - want.numpy())[diff].max(initial=0) <= 1
    assert torch.equal(cum.cpu(), got[:, 0].cumsum(1))
    assert torch.equal(yl.cpu(), got.sum((1, 2)).clamp_min(1).long())
    assert bad.item() == 0


@pytest.mark.parametrize("B,Tx", [(1, 1), (3, 37), (2, 300)])
def test_given_durations_with_zeros(B, Tx):
    from matcha_hip import runtime as rt
    from oracle import matcha_oracle as O
    _, x_mask, _, _ = _inputs(B, Tx, seed=Tx)
    g = torch.Generator().manual_seed(Tx + 1)
    d = torch.randint(0, 5, (B, Tx), generator=g)
    d[:, ::3] = 0
    d[B - 1] = 0  # one row with no frame at all
    w_ceil, cum, yl, bad = rt.durations(None, x_mask.to(DEV), durations=d.to(DEV))
    dm = d.float() * x_mask[:, 0]
    assert torch.equal(w_ceil.cpu(), dm[:, None])
    assert torch.equal(yl.cpu(), dm.sum(1).clamp_min(1).long()) and yl[B - 1].item() == 1
    assert torch.equal(cum.cpu(), dm.cumsum(1)) and bad.item() == 0
    t_pad = O.fix_len_compatibility(int(yl.max()))
    attn, _, y_mask = rt.alignment(cum, yl, t_pad, None)
    y_mask_o = O.sequence_mask(yl.cpu(), t_pad).unsqueeze(1).float()
    attn_o = O.generate_path(dm, (x_mask.unsqueeze(-1) * y_mask_o.unsqueeze(2)).squeeze(1))
    assert torch.equal(attn.cpu()[:, 0], attn_o) and torch.equal(y_mask.cpu(), y_mask_o)
    if B * Tx > 1:
        assert attn_o.sum() == dm.sum() > 0 and attn_o[B - 1].sum() == 0
    # a host tensor or nested lists are the same request
    again = rt.durations(None, x_mask.to(DEV), durations=d.tolist())
    assert torch.equal(again[1], cum)


@pytest.mark.parametrize("value", [-1.0, 2.5, float("nan"), float("inf"), 2.0 ** 24])
def test_bad_durations_set_the_flag(value):
    from matcha_hip import runtime as rt
    _, x_mask, _, _ = _inputs(3, 37, seed=37)  # rows of 37, 24 and 9 tokens
    d = torch.ones(3, 37)
    assert rt.durations(None, x_mask.to(DEV), durations=d)[3].item() == 0
    d[1, 30] = value  # past row 1's 24 tokens: masked, so it does not count
    d[2, 36] = -3.0
    if math.isfinite(value):  # (inf or NaN times the mask's 0 is NaN, which the row sum reports)
        assert rt.durations(None, x_mask.to(DEV), durations=d)[3].item() == 0
    d[1, 23] = value  # row 1's last token
    w_ceil, cum, yl, bad = rt.durations(None, x_mask.to(DEV), durations=d)
    assert bad.item() == 1
    with pytest.raises(ValueError):
        rt.durations(None, x_mask.to(DEV), 1.5, durations=torch.ones(3, 37))
    with pytest.raises(ValueError):
        rt.durations(None, x_mask.to(DEV), durations=torch.ones(3, 36))


def test_token_scale_that_overflows_sets_the_flag():
    from matcha_hip import runtime as rt
    logw, x_mask, ls, ts = _inputs(2, 300, seed=300)
    ts[0, 5] = 3e38
    assert rt.durations(logw.to(DEV), x_mask.to(DEV), ls, token_scale=ts)[3].item() == 1
    ts[0, 5] = -1.0
    assert rt.durations(logw.to(DEV), x_mask.to(DEV), ls, token_scale=ts)[3].item() == 1


# ---------------------------------------------------------------- 2. / 3. the model
@functools.lru_cache(maxsize=None)
def _matcha(prec):
    from matcha_hip import synthetic
    m = make_matcha(1, prec)
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in m.state_dict().items()], 5).items()}
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(24)
    x = torch.randint(1, 178, (3, 24), generator=g)
    xl = torch.tensor([24, 17, 9])
    return sd, m.to(DEV).eval(), x, xl


SEEDS = [3, -8, 2 ** 33]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_predicted_durations_round_trip(prec):
    """synthesize on its own predicted durations, and with a token scale of ones, is synthesize: the same bits"""
    sd, m, x, xl = _matcha(prec)
    base = m.synthesize(x.to(DEV), xl.to(DEV), 2, seeds=SEEDS)
    d = m.predict_durations(x.to(DEV), xl.to(DEV))
    assert d.dtype == torch.int64 and d.shape == (3, 24) and d.is_cuda
    assert torch.equal(d.sum(1), base[1]) and d[1, 17:].sum() == 0 and d[0].min() >= 1
    print(f"{prec}: durations {d[2, :9].tolist()}, y_lengths {base[1].tolist()}")
    for kw in (dict(durations=d), dict(durations=d.cpu().tolist()), dict(token_scale=torch.ones(3, 24))):
        out = m.synthesize(x.to(DEV), xl.to(DEV), 2, seeds=SEEDS, **kw)
        for u, v in zip(base, out):
            assert torch.equal(u, v), list(kw)
    out = m.synthesise(x.to(DEV), xl.to(DEV), 2, seeds=SEEDS, durations=d)
    assert torch.equal(out["mel"], base[0])
    # a length scale and a token scale reach predict_durations as they reach synthesize
    ts = torch.full((3, 24), 1.5)
    d2 = m.predict_durations(x.to(DEV), xl.to(DEV), length_scale=[1.0, 1.2, 0.9], token_scale=ts)
    out = m.synthesize(x.to(DEV), xl.to(DEV), 2, seeds=SEEDS, length_scale=[1.0, 1.2, 0.9], token_scale=ts)
    assert torch.equal(d2.sum(1), out[1]) and not torch.equal(d2, d)
    assert torch.equal(out[2][:, 0].sum(-1).long(), d2)


def test_edited_durations_against_the_oracle():
    """one token doubled, one dropped: y_lengths and attn exactly, the mel within the fp32 bar of the oracle's solve
    on generate_path of the same durations and the same seeded noise"""
    from matcha_hip import runtime as rt
    from oracle import matcha_oracle as O
    sd, m, x, xl = _matcha("fp32")
    d = m.predict_durations(x.to(DEV), xl.to(DEV)).cpu()
    d[0, 3] *= 2
    d[1, 5] = 0
    d[2, 0] += 3
    mel, yl, attn = m.synthesize(x.to(DEV), xl.to(DEV), 2, temperature=0.667, seeds=SEEDS, durations=d)
    assert torch.equal(yl.cpu(), d.sum(1))
    y_max = int(d.sum(1).max())
    t_pad = O.fix_len_compatibility(y_max)
    mu, _, x_mask = O.text_encoder(O.sub(sd, "encoder"), x, xl, dict(HP, n_spks=1))
    y_mask = O.sequence_mask(d.sum(1), t_pad).unsqueeze(1).float()
    attn_o = O.generate_path(d.float(), (x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)).squeeze(1))
    assert torch.equal(attn.cpu()[:, 0], attn_o) and attn_o[1, 5].sum() == 0
    mu_y = torch.matmul(attn_o.transpose(1, 2), mu.transpose(1, 2)).transpose(1, 2)
    z = rt.seeded_noise(torch.tensor(SEEDS, device=DEV), t_pad, temperature=0.667).cpu()
    mel_o = O.cfm_solve(O.sub(sd, "decoder.estimator"), mu_y, y_mask, 2, z, None, "euler", 2)
    mel_o = O.denormalize(mel_o, sd["mel_mean"], sd["mel_std"])[:, :, :y_max]
    err = (mel.cpu() - mel_o).abs().max().item()
    print(f"edited durations: mel max|d| {err:.3e}")
    assert mel.shape == mel_o.shape and err < 1e-4, err
    d[1, 2] = -1
    with pytest.raises(ValueError):
        m.synthesize(x.to(DEV), xl.to(DEV), 2, seeds=SEEDS, durations=d)
