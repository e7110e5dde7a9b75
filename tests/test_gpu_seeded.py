"""Per-utterance seeds, temperature and length scale (MI355X): the seeded noise kernel against its CPU specification
(matcha_hip/noise.py), its independence from the batch, the fused draw inside the CFM solve against the standalone
op, per-row durations, and synthesize end to end against the oracle."""
import numpy as np
import pytest
import torch

from conftest import HP, golden, make_decoder, make_matcha, t, weights_from

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = [0, 1, 2 ** 63 - 1, -1, -2 ** 63]


def _load(mod, sd):
    mod.load_state_dict(sd)
    return mod.to(DEV).eval()


def _seeds(vals):
    return torch.tensor(list(vals), dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- 1. the stream
@pytest.mark.parametrize("temps", [None, [0.3, 0.667, 1.0]])
@pytest.mark.parametrize("B,T", [(1, 2), (3, 46), (2, 730)])
def test_stream_matches_cpu_specification(B, T, temps):
    """The tolerance comes from the references alone: 8 x max|ref32 - ref64|, ref32 the same formula in numpy float32
    on the same counters (numpy's log / sin / cos are <= 1 ulp, the device's a few, at r <= 5.77)."""
    from matcha_hip import runtime as rt
    from matcha_hip.noise import reference_noise
    seeds = SEEDS[:B]
    tau = None if temps is None else np.asarray(temps[:B], dtype=np.float32)
    ref64 = np.stack([reference_noise(s, T) for s in seeds])
    ref32 = np.stack([reference_noise(s, T, dtype=np.float32) for s in seeds])
    if tau is not None:
        ref64 = ref64 * tau.astype(np.float64)[:, None, None]
        ref32 = ref32 * tau[:, None, None]
    assert ref32.dtype == np.float32
    tol = 8 * np.abs(ref32.astype(np.float64) - ref64).max()
    z = rt.seeded_noise(_seeds(seeds), T, temperature=None if tau is None else list(temps[:B]))
    assert z.shape == (B, 80, T) and z.dtype == torch.float32 and z.is_cuda
    dev = np.abs(z.cpu().numpy().astype(np.float64) - ref64).max()
    print(f"B={B} T={T} temps={temps}: GPU max|d| {dev:.3e}, tol {tol:.3e}")
    assert dev <= tol, (dev, tol)


def test_stream_other_channel_counts():
    """C is any multiple of 4; fewer channels are a prefix of more (the counter holds c // 4)"""
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    s = _seeds([5, 6])
    a, b = rt.seeded_noise(s, 33, C=8), rt.seeded_noise(s, 33, C=80)
    assert a.shape == (2, 8, 33) and torch.equal(a, b[:, :8])
    with pytest.raises(HipPathError, match="C 6"):
        rt.seeded_noise(s, 33, C=6)


# ---------------------------------------------------------------- 2. independence from the batch
def test_stream_is_independent_of_the_batch():
    from matcha_hip import runtime as rt
    big = rt.seeded_noise(_seeds(SEEDS), 108)
    rev = rt.seeded_noise(_seeds(SEEDS[::-1]), 108)
    for p, s in enumerate(SEEDS):
        one = rt.seeded_noise(_seeds([s]), 46)
        assert torch.equal(one[0], big[p][:, :46]), s
        assert torch.equal(one[0], rev[len(SEEDS) - 1 - p][:, :46]), s
    assert not torch.equal(big[0], big[1])
    # a scaled row is the unscaled row times its own temperature, one fp32 multiply
    tau = torch.tensor([0.3, 0.667, 1.0, 1.5, 0.0], device=DEV)
    assert torch.equal(rt.seeded_noise(_seeds(SEEDS), 108, temperature=tau), big * tau[:, None, None])


# ---------------------------------------------------------------- 3. / 4. the fused draw inside the solve
@pytest.fixture(scope="module", params=[("fp32", 160), ("bf16", 160), ("fp32", 224), ("bf16", 224)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def decoder(request):
    from matcha_hip import synthetic
    prec, c_cond = request.param
    dec = make_decoder(c_cond, prec)
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in dec.state_dict().items()], 41).items()}
    dec = _load(dec, sd)
    yield dec, c_cond
    dec.engine().set_graphs(1)


def _solve_inputs(T, lens, c_cond):
    g = torch.Generator().manual_seed(T)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()[:, None]
    mu = torch.randn(len(lens), 80, T, generator=g) * mask
    spks = torch.randn(len(lens), 64, generator=g).to(DEV) if c_cond == 224 else None
    return mu.to(DEV), mask.to(DEV), spks


# T = 48: one row unpadded (the general attention path); T = 108: every row padded, at both U-Net levels (with
# max_valid the bf16 solver takes the query-independent attention path)
SOLVE_CASES = [(48, [48, 30, 17]), (108, [105, 76, 46])]


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_seeded_solve_equals_solve_on_seeded_noise(decoder, solver):
    """solve(seeds=...) draws the noise straight into the solver's two workspace layouts; bit for bit it is the solve
    on z_noise = seeded_noise(...), for one shared temperature (applied by the solve's transpose) and for one per
    row (applied by the generator)."""
    from matcha_hip import runtime as rt
    dec, c_cond = decoder
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    seeds = _seeds([11, -5, 2 ** 40])
    tau_b = torch.tensor([0.667, 0.3, 1.0], device=DEV)
    try:
        for (T, lens), graphs in [(c, g) for c in SOLVE_CASES for g in (1, 0)]:
            eng.set_graphs(graphs)
            mu, mask, spks = _solve_inputs(T, lens, c_cond)
            kw = dict(solver=solver, max_valid=max(lens))
            a = eng.solve(pk, None, 0.667, mu, mask, spks, 2, seeds=seeds, **kw)
            b = eng.solve(pk, rt.seeded_noise(seeds, T), 0.667, mu, mask, spks, 2, **kw)
            assert torch.isfinite(a).all()
            assert torch.equal(a, b), (T, graphs, (a - b).abs().max().item())
            c = eng.solve(pk, None, tau_b, mu, mask, spks, 2, seeds=seeds, **kw)
            d = eng.solve(pk, rt.seeded_noise(seeds, T, temperature=tau_b), 1.0, mu, mask, spks, 2, **kw)
            assert torch.equal(c, d), (T, graphs, (c - d).abs().max().item())
            assert not torch.equal(a, c)
            # a sequence of ints is the same request as the tensor
            assert torch.equal(eng.solve(pk, None, 0.667, mu, mask, spks, 2, seeds=[11, -5, 2 ** 40], **kw), a)
    finally:
        eng.set_graphs(1)


def test_seeded_solve_graph_replay(decoder):
    """the noise kernel runs outside the captured chain: a replay with other seeds gives another result, and each
    equals its direct-launch twin"""
    dec, c_cond = decoder
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    T, lens = SOLVE_CASES[1]
    mu, mask, spks = _solve_inputs(T, lens, c_cond)
    s1, s2 = _seeds([1, 2, 3]), _seeds([4, 5, 6])

    def run(graphs, seeds):
        eng.set_graphs(graphs)
        return eng.solve(pk, None, 0.667, mu, mask, spks, 3, seeds=seeds, max_valid=max(lens))

    try:
        g1, g2 = run(1, s1), run(1, s2)  # capture (or a cached graph), then a replay
        d1, d2 = run(0, s1), run(0, s2)
        assert not torch.equal(g1, g2)
        assert torch.equal(g1, d1) and torch.equal(g2, d2)
        assert torch.equal(run(1, s1), g1)
    finally:
        eng.set_graphs(1)


def test_solve_argument_errors(decoder):
    dec, c_cond = decoder
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    mu, mask, spks = _solve_inputs(*SOLVE_CASES[0], c_cond)
    with pytest.raises(TypeError):
        eng.solve(pk, None, 1.0, mu, mask, spks, 2, seeds=7)
    with pytest.raises(ValueError):
        eng.solve(pk, None, 1.0, mu, mask, spks, 2, seeds=[1, 2])
    with pytest.raises(ValueError):
        eng.solve(pk, None, torch.ones(4), mu, mask, spks, 2, seeds=[1, 2, 3])
    with pytest.raises(TypeError):
        eng.solve(pk, torch.zeros_like(mu), torch.ones(3), mu, mask, spks, 2)


# ---------------------------------------------------------------- 5. per-row durations
def test_durations_per_row_golden():
    from matcha_hip import runtime as rt
    g = golden("g1_durations")
    logw, x_mask = t(g["logw"], DEV), t(g["x_mask"], DEV)
    ls0, ls1 = float(g["ls0"]), float(g["ls1"])
    scal = [rt.durations(logw, x_mask, ls) for ls in (ls0, ls1)]
    pick = [0, 1, 0]
    for ls in ([ls0, ls1, ls0], torch.tensor([ls0, ls1, ls0]), torch.tensor([ls0, ls1, ls0], device=DEV)):
        w_ceil, cum, yl = rt.durations(logw, x_mask, ls)
        for b, i in enumerate(pick):
            assert torch.equal(w_ceil[b].cpu(), t(g[f"w_ceil{i}"])[b])
            assert torch.equal(cum[b], scal[i][1][b])
        assert yl.tolist() == [107, 76, 46]
    with pytest.raises(ValueError):
        rt.durations(logw, x_mask, [1.0, 1.0])


def test_durations_per_row_long_text():
    """Tx past the scan's 8192-token chunk: each row is the unchanged scalar call on that row alone"""
    from matcha_hip import runtime as rt
    B, Tx = 2, 20001
    g = torch.Generator().manual_seed(Tx)
    logw = (torch.randn(B, 1, Tx, generator=g) * 0.7 + 0.6).to(DEV)
    lens = torch.tensor([Tx, 15000])
    x_mask = (torch.arange(Tx)[None] < lens[:, None]).float()[:, None].to(DEV)
    scales = [0.7, 1.3]
    w_ceil, cum, yl = rt.durations(logw, x_mask, scales)
    for b, ls in enumerate(scales):
        w1, c1, y1 = rt.durations(logw[b:b + 1], x_mask[b:b + 1], ls)
        assert torch.equal(w_ceil[b:b + 1], w1) and torch.equal(cum[b:b + 1], c1) and torch.equal(yl[b:b + 1], y1)
    assert yl[0] != yl[1]


# ---------------------------------------------------------------- 6. end to end
def _g6_model(tag):
    g = golden(f"g6_synth_{tag}")
    sd = weights_from(g)
    sd["encoder.proj_w.proj.weight"] = t(g["proj_w_weight"])
    sd["encoder.proj_w.proj.bias"] = t(g["proj_w_bias"])
    m = _load(make_matcha(1 if tag == "lj" else 109, "fp32"), sd)
    spks = t(g["spks"]) if g["spks"].size else None
    return g, sd, m, spks


@pytest.mark.parametrize("tag", ["lj", "vctk"])
def test_synthesize_seeded_end_to_end_fp32(tag):
    """B = 2 with a seed, a temperature and a length scale per utterance: the index path bit for bit against the
    oracle's align run per row with that row's scale, the mel against the oracle's solve fed the seeded noise, within
    test_synthesize_end_to_end_fp32's bar."""
    from matcha_hip import runtime as rt
    from oracle import matcha_oracle as O
    g, sd, m, spks = _g6_model(tag)
    x, xl = t(g["x"]), t(g["x_lengths"])
    seeds, temps, scales = [7, -3], [0.667, 0.3], [1.0, 0.85]
    mel, yl, attn = m.synthesize(x.to(DEV), xl.to(DEV), n_timesteps=4, temperature=temps,
                                 spks=None if spks is None else spks.to(DEV), length_scale=scales, seeds=seeds)
    hp = dict(HP, n_spks=1 if tag == "lj" else 109)
    mu, logw, x_mask = O.text_encoder(O.sub(sd, "encoder"), x, xl, hp, spks)
    rows = [O.align(logw[b:b + 1], x_mask[b:b + 1], mu[b:b + 1], scales[b]) for b in range(2)]
    yl_o = torch.cat([r[0] for r in rows])
    assert torch.equal(yl.cpu(), yl_o)
    assert yl_o[0] != yl_o[1]
    y_max = int(yl_o.max())
    t_pad = O.fix_len_compatibility(y_max)
    assert attn.shape == (2, 1, x.shape[1], t_pad) and mel.shape == (2, 80, y_max)
    mu_y = torch.zeros(2, 80, t_pad)
    for b, (_, _, tp_b, _, attn_b, mu_y_b) in enumerate(rows):
        assert torch.equal(attn[b:b + 1, :, :, :tp_b].cpu(), attn_b)
        assert attn[b, :, :, tp_b:].abs().sum() == 0
        mu_y[b, :, :tp_b] = mu_y_b[0]
    y_mask = O.sequence_mask(yl_o, t_pad).unsqueeze(1).float()
    z = rt.seeded_noise(_seeds(seeds), t_pad, temperature=temps).cpu()
    mel_o = O.cfm_solve(O.sub(sd, "decoder.estimator"), mu_y, y_mask, 4, z, spks, "euler", hp.get("heads", 2))
    mel_o = O.denormalize(mel_o, sd["mel_mean"], sd["mel_std"])[:, :, :y_max]
    err = (mel.cpu() - mel_o).abs().max().item()
    print(f"{tag}: seeded end to end mel max|d| {err:.3e}")
    assert err < 2e-4, f"{tag}: mel max|d|={err:.3e}"
    # the same request again, as tensors and through the dict alias: the same bits
    out = m.synthesise(x.to(DEV), xl.to(DEV), 4, torch.tensor(temps), None if spks is None else spks.to(DEV),
                       torch.tensor(scales), _seeds(seeds))
    assert torch.equal(out["mel"], mel) and torch.equal(out["mel_lengths"], yl)


# ---------------------------------------------------------------- 7. scalars are untouched
def test_uniform_per_row_arguments_equal_the_scalar_call(monkeypatch):
    g, sd, m, spks = _g6_model("lj")
    z = t(g["z"], DEV)
    monkeypatch.setattr(torch, "randn_like", lambda ref, *a, **k: z.clone())
    x, xl = t(g["x"], DEV), t(g["x_lengths"], DEV)
    B = x.shape[0]
    a = m.synthesize(x, xl, n_timesteps=4, temperature=0.667, length_scale=1.0)
    b = m.synthesize(x, xl, n_timesteps=4, temperature=torch.full((B,), 0.667), length_scale=torch.ones(B))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # and the scalar call is still the reference's result
    assert torch.equal(a[1].cpu(), t(g["y_lengths"]))
    assert (a[0].cpu() - t(g["mel"])).abs().max() < 2e-4


# ---------------------------------------------------------------- 8. errors
def test_synthesize_argument_errors():
    g, sd, m, spks = _g6_model("lj")
    x, xl = t(g["x"], DEV), t(g["x_lengths"], DEV)
    with pytest.raises(TypeError):
        m.synthesize(x, xl, n_timesteps=2, seeds=7)
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=2, seeds=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=2, seeds=[1, 2], temperature=torch.ones(3))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=2, length_scale=torch.ones(1))
    with pytest.raises(TypeError):
        m.decoder(torch.zeros(2, 80, 8, device=DEV), torch.ones(2, 1, 8, device=DEV), 2, seeds=3)
