"""Multi-speaker training step (n_spks = 109, spk_emb_dim = 64) on the GPU: the two speaker-path primitives
(mtt_bcast_cols, mtt_segsum_cols) op by op, and the whole step / the Lightning drop-in against torch autograd
through the oracle, composed here with the speaker vector (train_standalone.py:623-667: the oracle's own
training_losses is single speaker)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import HP, make_matcha
from matcha_hip import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SPKS, E = 109, 64
HPS = dict(HP, n_spks=N_SPKS)
IDS = (5, 108, 5)  # a repeated speaker: two utterances accumulate into one table row


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _weights(n_spks, seed):
    m = make_matcha(n_spks, "fp32")
    return {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed).items()}


def _batch(seed=21, B=3, Tx=17, Ty=64, x_len=(17, 12, 9), y_len=(64, 50, 33)):
    """the batch of test_gpu_train._setup"""
    g = torch.Generator().manual_seed(seed)
    xl, yl = torch.tensor(x_len), torch.tensor(y_len)
    x = torch.randint(1, 178, (B, Tx), generator=g) * (torch.arange(Tx)[None] < xl[:, None])
    y = torch.randn(B, 80, Ty, generator=g) * 1.5 * (torch.arange(Ty)[None, None] < yl[:, None, None])
    t = torch.rand(B, generator=g)
    z = torch.randn(B, 80, Ty, generator=g)
    return x, xl, y, yl, t, z


def _spk_losses(sd, ids, x, xl, y, yl, t, z, hp, mas=None, sigma_min=1e-4):
    """train_standalone.py:623-667 with spks = self.spk_emb(ids) (:626) fed to the encoder (:631) and to
    compute_loss (:658); otherwise oracle.training_losses line for line. hp without n_spks > 1: single speaker."""
    import oracle.matcha_oracle as O
    multi = hp.get("n_spks", 1) > 1
    spks = F.embedding(ids, sd["spk_emb.weight"]) if multi else None
    n_feats = y.shape[1]
    mu_x, logw, x_mask = O.text_encoder(O.sub(sd, "encoder"), x, xl, hp, spks)
    y_mask = O.sequence_mask(yl, y.shape[-1]).unsqueeze(1).to(x_mask)
    attn_mask = x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)
    with torch.no_grad():
        const = -0.5 * math.log(2 * math.pi) * n_feats
        factor = -0.5 * torch.ones(mu_x.shape, dtype=mu_x.dtype, device=mu_x.device)
        y_square = torch.matmul(factor.transpose(1, 2), y ** 2)
        y_mu_double = torch.matmul(2.0 * (factor * mu_x).transpose(1, 2), y)
        mu_square = torch.sum(factor * (mu_x ** 2), 1).unsqueeze(-1)
        log_prior = y_square - y_mu_double + mu_square + const
        attn = (mas or O.maximum_path)(log_prior, attn_mask.squeeze(1)).to(y.device)
    logw_ = torch.log(1e-8 + torch.sum(attn.unsqueeze(1), -1)) * x_mask
    dur_loss = torch.sum((logw - logw_) ** 2) / torch.sum(xl)
    mu_y = torch.matmul(attn.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    tt = t.view(-1, 1, 1)
    y_t = (1 - (1 - sigma_min) * tt) * z + tt * y
    u_t = y - (1 - sigma_min) * z
    pred = O.decoder_forward(O.sub(sd, "decoder.estimator"), y_t, y_mask, mu_y, t, spks=spks)
    cfm_loss = F.mse_loss(pred, u_t, reduction="sum") / (torch.sum(y_mask) * u_t.shape[1])
    prior_loss = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask)
    prior_loss = prior_loss / (torch.sum(y_mask) * n_feats)
    return dur_loss, prior_loss, cfm_loss, attn, log_prior


def _trained(k):
    return k == "spk_emb.weight" or k.startswith(("encoder.", "decoder.estimator."))


def _oracle_grads(sd, ids, batch, hp, mas=None, dev="cpu", dt=None, scale=1.0):
    """fp32 autograd through the composed oracle (under torch.autocast(dt) on the GPU when dt is given) ->
    (dur, prior, cfm, attn, log_prior), gradients / scale by name"""
    params = {k: v.clone().float().to(dev).requires_grad_(True) for k, v in sd.items()
              if _trained(k) and (k != "spk_emb.weight" or hp.get("n_spks", 1) > 1)}
    args = [v.to(dev) for v in batch]
    if dt is None:
        out = _spk_losses(params, ids.to(dev), *args, hp, mas=mas)
    else:
        with torch.autocast("cuda", dtype=dt):
            out = _spk_losses(params, ids.to(dev), *args, hp, mas=mas)
    grads = torch.autograd.grad((out[0] + out[1] + out[2]) * scale, list(params.values()), allow_unused=True)
    return out, {k: ((gr.float() / scale) if gr is not None else torch.zeros_like(p)).cpu()
                 for (k, p), gr in zip(params.items(), grads)}


@functools.lru_cache(maxsize=None)
def _case():
    """weights, ids, batch and the fp32 CPU oracle's losses and gradients, computed once for the module"""
    sd = _weights(N_SPKS, 21)
    ids, batch = torch.tensor(IDS), _batch()
    out, gref = _oracle_grads(sd, ids, batch, HPS)
    return sd, ids, batch, tuple(v.detach() for v in out), gref


def _gpu_step(sd, ids, batch, hp=HPS, loss_scale=None, **kw):
    from matcha_hip.train import MatchaTrainer
    x, xl, y, yl, t, z = (v.to(DEV) for v in batch)
    tr = MatchaTrainer(sd, hp, DEV, dropout=False, **kw)
    if tr.scaler is not None and loss_scale is not None:
        tr.scaler["scale"] = loss_scale
    out = tr.forward_backward(x, xl, y, yl, t=t, z=z, spks=None if ids is None else ids.to(DEV))
    torch.cuda.synchronize()
    return tr, out


# ------------------------------------------------------------------------------------------- primitives
@pytest.mark.parametrize("B,seg,n,ldd,doff", [(3, 5, 64, 224, 160), (2, 1, 1, 3, 2), (3, 513, 65, 130, 65)])
def test_bcast_cols(B, seg, n, ldd, doff):
    """mtt_bcast_cols: exactly src.repeat_interleave(seg, 0) in the column slice, every other column untouched"""
    from matcha_hip import train as T
    g = torch.Generator().manual_seed(1)
    src = torch.randn(B, n, generator=g).to(DEV)
    dst = torch.full((B, seg, ldd), -7.5, device=DEV)
    T.bcast_cols(src, dst, doff, seg)
    torch.cuda.synchronize()
    want = torch.full((B * seg, ldd), -7.5, device=DEV)
    want[:, doff:doff + n] = src.repeat_interleave(seg, 0)
    assert torch.equal(dst.view(B * seg, ldd), want)


@pytest.mark.parametrize("seg,n,soff,accumulate", [(1, 1, 0, 0), (3, 64, 160, 0), (64, 64, 160, 1), (512, 65, 0, 0),
                                                   (513, 65, 3, 1), (1030, 64, 192, 0)])
def test_segsum_cols(seg, n, soff, accumulate):
    """mtt_segsum_cols against the fp64 sum of the slice. Bound per element: seg * 2^-24 * sum_r |a[r][j]|, the
    worst case of fp32 summation in ANY order (each of the < seg adds rounds by at most 2^-24 of a partial sum
    that the sum of magnitudes bounds), plus 2^-24 |out| for the one extra add when accumulating. A second call
    on the same input is bit-identical (fixed-order reduction, no atomics)."""
    from matcha_hip import train as T
    B, lda = 3, soff + n + 7
    g = torch.Generator().manual_seed(seg * 131 + n)
    a = torch.randn(B, seg, lda, generator=g).to(DEV)
    out0 = torch.randn(B, n, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        out = out0.clone()
        T.segsum_cols(a, soff, n, seg, out, acc=bool(accumulate))
        outs.append(out)
    torch.cuda.synchronize()
    sl = a[:, :, soff:soff + n].double()
    want = sl.sum(1) + (out0.double() if accumulate else 0.0)
    bound = seg * 2.0 ** -24 * sl.abs().sum(1)
    if accumulate:
        bound = bound + 2.0 ** -24 * want.abs()
    err = (outs[0].double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------------------------- the step
def test_multi_speaker_step_matches_autograd():
    """The fp32 multi-speaker step against fp32 autograd through the composed oracle, with the bars of
    test_gpu_train._check_step (attn equal, log-prior rel 1e-5, losses rel 1e-4, per-tensor gradient rel-L2 2e-3
    with the conv_k.bias exception, flat gradient 5e-4), plus the speaker table on its own: rel-L2 < 2e-3 and every
    row but 5 and 108 exactly zero (the table is ~5e-4 of the flat gradient's norm: the flat check cannot see it).
    buckets.finish() inside forward_backward is the marked-exactly-once check."""
    sd, ids, batch, (dur, prior, cfm, attn, lp), gref = _case()
    tr, out = _gpu_step(sd, ids, batch)
    assert torch.equal(out["attn"].cpu(), attn.float())
    assert _rel(out["log_prior"], lp) < 1e-5
    for name, a, b in (("dur", out["dur_loss"], dur), ("prior", out["prior_loss"], prior), ("cfm", out["cfm_loss"], cfm)):
        assert abs(a.item() - b.item()) <= 1e-4 * abs(b.item()), (name, a.item(), b.item())
    got = tr.gradients()
    assert set(got) == set(gref) and tr.grads.names[-1] == "spk_emb.weight"
    kb = [k for k in gref if k.endswith("conv_k.bias")]
    for k in kb:
        assert float((got[k].cpu() - gref[k]).norm()) <= 1e-3 * float(gref[k[:-4] + "weight"].norm()), k
    worst = max((_rel(got[k], gref[k]), k) for k in gref if k not in kb)
    assert worst[0] < 2e-3, worst
    flat_ref = torch.cat([gref[n].reshape(-1) for n in tr.grads.names])
    assert _rel(tr.grads.flat, flat_ref) < 5e-4
    gt = got["spk_emb.weight"].cpu()
    assert _rel(gt, gref["spk_emb.weight"]) < 2e-3
    others = [r for r in range(N_SPKS) if r not in IDS]
    assert bool((gt[others] == 0).all()) and all(float(gt[r].norm()) > 0 for r in set(IDS))


def test_speaker_argument_errors():
    """n_spks = 109 without ids: ValueError; an id outside [0, 109): IndexError; a single-speaker trainer ignores
    spks (train_standalone.py:625-628): bit-identical losses and gradients with and without them."""
    from matcha_hip.train import MatchaTrainer
    sd, ids, batch, _, _ = _case()
    x, xl, y, yl, t, z = (v.to(DEV) for v in batch)
    tr = MatchaTrainer(sd, HPS, DEV, dropout=False)
    with pytest.raises(ValueError, match="spks"):
        tr.forward_backward(x, xl, y, yl, t=t, z=z)
    for bad in (109, -1):
        with pytest.raises(IndexError, match="speaker id"):
            tr.forward_backward(x, xl, y, yl, t=t, z=z, spks=torch.tensor([5, bad, 5], device=DEV))
    sd1 = _weights(1, 21)
    res = []
    for spks in (None, ids):
        tr1, out = _gpu_step(sd1, spks, batch, hp=HP)
        res.append(([out[k].item() for k in ("dur_loss", "prior_loss", "cfm_loss")], tr1.grads.flat.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


# -------------------------------------------------------------------------------------- mixed precision
MIXED_IDS = (5, 108, 5, 0, 77, 108, 31, 5)


def _mixed_batch(seed=31, B=8, Tx=40, Ty=160):
    """B = 8, T_x = 40, T_y = 160, ragged lengths (the longest utterance full), ~3.2-4 frames per token"""
    rs = np.random.RandomState(seed)
    xl = rs.randint(15, Tx + 1, B)
    xl[0] = Tx
    yl = np.minimum(Ty, np.round(xl * rs.uniform(3.2, 4.0, B))).astype(int)
    yl[0] = Ty
    return _batch(seed=seed, B=B, Tx=Tx, Ty=Ty, x_len=tuple(int(v) for v in xl), y_len=tuple(int(v) for v in yl))


@functools.lru_cache(maxsize=None)
def _mixed_ref(n_spks=N_SPKS):
    """weights, ids, batch, the fp32 GPU run's alignment and the fp32 CPU oracle on that alignment, computed once"""
    sd, ids, batch = _weights(n_spks, 21), torch.tensor(MIXED_IDS), _mixed_batch()
    hp = HPS if n_spks > 1 else HP
    ref, out = _gpu_step(sd, ids, batch, hp=hp)
    attn = out["attn"].cpu()
    del ref
    (dur, prior, cfm, _, _), gref = _oracle_grads(sd, ids, batch, hp, mas=lambda lp, m: attn)
    return sd, ids, batch, hp, attn, [float(v.detach()) for v in (dur, prior, cfm)], gref


def _mixed_vs_autocast(ref, precision, dt):
    """-> (flat-gradient error of this trainer, of the oracle under autocast; the three losses of this trainer,
    of autocast, of the fp32 oracle), all on the fp32 run's alignment. fp16 on both sides with GradScaler's rule:
    the loss scale starts at 2^16 and halves until the gradient is finite."""
    sd, ids, batch, hp, attn, l_ref, gref = ref
    fixed = lambda lp, m: attn.to(lp.device)  # noqa: E731
    S = 65536.0 if dt == torch.float16 else 1.0
    while True:
        tr, out = _gpu_step(sd, ids, batch, hp=hp, precision=precision, loss_scale=S)
        mine = tr.grads.flat.detach().double().cpu() / S
        if torch.isfinite(mine).all() or S < 1.0:
            break
        S /= 2.0
    assert torch.isfinite(mine).all()
    assert torch.equal(out["attn"].cpu(), attn)
    names = list(tr.grads.names)
    flat_ref = torch.cat([gref[n].reshape(-1) for n in names]).double()
    ac_S = 65536.0 if dt == torch.float16 else 1.0
    while True:
        ac_out, ac_g = _oracle_grads(sd, ids, batch, hp, mas=fixed, dev=DEV, dt=dt, scale=ac_S)
        if all(torch.isfinite(v).all() for v in ac_g.values()) or ac_S < 1.0:
            break
        ac_S /= 2.0
    flat_ac = torch.cat([ac_g[n].reshape(-1) for n in names]).double()
    l_mine = [float(out[k]) for k in ("dur_loss", "prior_loss", "cfm_loss")]
    l_ac = [float(v.detach()) for v in ac_out[:3]]
    return _rel(mine, flat_ref), _rel(flat_ac, flat_ref), l_mine, l_ac, l_ref, ac_S


@pytest.mark.parametrize("precision,dt", [("16-mixed", torch.float16), ("bf16-mixed", torch.bfloat16)])
def test_multi_speaker_mixed_precision_vs_autocast(precision, dt):
    """The multi-speaker step with 16-bit GEMM operands against the fp32 autograd oracle, alignment fixed to the
    fp32 run's: the rule of test_training_step_mixed_precision_vs_autocast: the flat gradient no further from fp32
    than the composed oracle under torch.autocast on the GPU x 1.25, each loss within max(1.5 x autocast's error,
    half the operand format's unit roundoff).

    Shape: B = 8, T_x = 40, T_y = 160, ids (5, 108, 5, 0, 77, 108, 31, 5). Measured there (flat gradient, this
    trainer vs autocast): 16-mixed 6.82e-3 vs 7.23e-3 (ratio 0.94), bf16-mixed 3.07e-2 vs 3.37e-2 (0.91); the
    single-speaker trainer at the same shape 6.83e-3 vs 8.37e-3 (0.82) and 1.09e-2 vs 2.26e-2 (0.48). At the fp32
    test's batch (B = 3, T_y = 64) the rule is not stable: 16-mixed 1.50e-2 vs 1.57e-2 / 2.73e-2 in two runs,
    bf16-mixed 6.50e-2 vs 5.38e-2 / 5.23e-2 (ratio 1.21 / 1.24 against the 1.25: autocast's own error moves by a
    few per cent from run to run, its backward is not bitwise reproducible), while the single-speaker trainer gave
    0.96 and 0.25 there. With 147 frames each error is one draw of rounding noise, not a rate; the batch was grown
    until both trainers sit clear of the factor, which stays 1.25."""
    e_mine, e_ac, l_mine, l_ac, l_ref, ac_S = _mixed_vs_autocast(_mixed_ref(), precision, dt)
    print(f"{precision}: flat {e_mine:.3e} vs autocast {e_ac:.3e} (scale {ac_S}); losses "
          f"{[abs(a - b) / abs(b) for a, b in zip(l_mine, l_ref)]} vs {[abs(a - b) / abs(b) for a, b in zip(l_ac, l_ref)]}")
    assert e_mine <= 1.25 * e_ac, (e_mine, e_ac)
    floor = 2.0 ** -12 if dt == torch.float16 else 2.0 ** -9
    for a_, c_, r_ in zip(l_mine, l_ac, l_ref):
        assert abs(a_ - r_) <= max(1.5 * abs(c_ - r_), floor * abs(r_)), (a_, c_, r_)


# ------------------------------------------------------------------------------------------ the drop-in
def _lightning(sd, table):
    from types import SimpleNamespace

    import train_standalone as TS
    from conftest import DEC, DP, ENC
    mod = TS.MatchaLightningModule(178, N_SPKS, E, SimpleNamespace(**ENC), SimpleNamespace(**DEC),
                                   {"solver": "euler", "sigma_min": 1e-4}, SimpleNamespace(**DP),
                                   {"mel_mean": 0.0, "mel_std": 1.0})
    mod.model.load_state_dict(sd)
    mod.spk_emb.load_state_dict({"weight": table})
    return mod.to(DEV)


def test_lightning_module_multi_speaker_drop_in():
    """MatchaLightningModule(n_spks = 109) with batch["spks"]: the step looks the ids up in, and trains, the
    module-level table (train_standalone.py:604-605, 626); model.spk_emb.weight gets no gradient, no Adam state
    and stays as loaded. validation_step matches the composed oracle on the module-level table (rel 1e-4); after
    one step only rows 5 and 108 of the table moved (zero gradient and zero moments: a zero first Adam update);
    module + optimizer state saved after step 1 and loaded into a fresh pair give a bit-identical step 2."""
    sd, ids, (x, xl, y, yl, _, _), _, _ = _case()
    table = torch.from_numpy(synthetic.make_state_dict([("spk_emb.weight", (N_SPKS, E))], 77)["spk_emb.weight"])
    assert not torch.equal(table, sd["spk_emb.weight"])
    mod = _lightning(sd, table)
    batch = {"x": x.to(DEV), "x_lengths": xl.to(DEV), "y": y.to(DEV), "y_lengths": yl.to(DEV), "spks": ids.to(DEV)}
    torch.manual_seed(99)
    t = torch.rand([3, 1, 1], device=DEV)
    z = torch.randn_like(batch["y"])
    torch.manual_seed(99)
    val = mod.validation_step(batch, 0).item()
    (dur, prior, cfm, _, _), _ = _oracle_grads(dict(sd, **{"spk_emb.weight": table}), ids,
                                               (x, xl, y, yl, t.view(3).cpu(), z.cpu()), HPS)
    ref = (dur + prior + cfm).item()
    assert abs(val - ref) <= 1e-4 * abs(ref), (val, ref)
    # one training step
    opt = mod.configure_optimizers()
    torch.manual_seed(1)
    loss = mod.training_step(batch, 0)
    assert math.isfinite(loss.item())
    opt.step()
    opt.zero_grad()
    w = mod.spk_emb.weight.detach().cpu()
    moved = [r for r in range(N_SPKS) if not torch.equal(w[r], table[r])]
    assert moved == sorted(set(IDS)), moved
    assert torch.equal(mod.model.spk_emb.weight.detach().cpu(), sd["spk_emb.weight"])
    assert torch.equal(mod.spk_emb.weight.detach(), mod.trainer().parameters()["spk_emb.weight"])
    names = [n for n, _ in mod.named_parameters()]
    osd = opt.state_dict()
    assert len(osd["state"]) == len(names) - 1 and names.index("model.spk_emb.weight") not in osd["state"]
    assert 0 in osd["state"] and names[0] == "spk_emb.weight"
    # resume: state saved after step 1 into a fresh module and optimizer
    msd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    torch.manual_seed(2)
    la = mod.training_step(batch, 1).item()
    opt.step()
    wa = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    b = _lightning(sd, sd["spk_emb.weight"])
    b.load_state_dict(msd)
    opt_b = b.configure_optimizers()
    opt_b.load_state_dict(osd)
    torch.manual_seed(2)
    lb = b.training_step(batch, 1).item()
    opt_b.step()
    assert la == lb
    for k, v in b.state_dict().items():
        assert torch.equal(v, wa[k]), k
