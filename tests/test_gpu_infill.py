"""Mel infill (MI355X, mt_cfm_solve_infill): kept frames are held on the conditional path p(t) = (1 - (1 - sigma_min) t)
z0 + t x1 while the CFM solve fills the others. Against a reference loop over the CPU oracle's estimator with the same
clamps, the exact identities (kept frames are x1's bits, nothing kept is the plain solve), the launch log, synthesize
end to end and MatchaTTS.edit.

Fixtures as in test_gpu_solve_rows.py: synthetic decoder weights (seed 41), counts in caller order [3, 5, 1, 3],
T = 48 (an unpadded row: general attention) and T = 108 (every row padded: query-independent attention; 108 frames x
20 four-channel groups do not fill the last 256-thread workgroup). Keep patterns: row 0 frames 8-19, row 1 everything,
row 2 frames 0-4 and 12 to the end of the buffer (padded frames included, which must be ignored), row 3 nothing."""
import pytest
import torch

from conftest import golden, make_decoder, make_matcha, rel_rms, t, weights_from

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = [3, 5, 1, 3]
CASES = [(48, [48, 30, 17, 40]), (108, [105, 76, 46, 90])]
CASE_IDS = ["T48-general", "T108-uniform"]
SOLVERS = ["euler", "midpoint"]
SIGMA = 1e-4

_DECODERS = {}
_REFS = {}  # CPU oracle results, computed once and shared (never modified)


def _decoder(prec, c_cond):
    from matcha_hip import synthetic
    if (prec, c_cond) not in _DECODERS:
        dec = make_decoder(c_cond, prec)
        sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
            [(k, tuple(v.shape)) for k, v in dec.state_dict().items()], 41).items()}
        dec.load_state_dict(sd)
        _DECODERS[prec, c_cond] = (dec.to(DEV).eval(), sd)
    return _DECODERS[prec, c_cond]


@pytest.fixture(scope="module")
def decoder_bf16_spk():
    dec, sd = _decoder("bf16", 224)
    yield dec, 224, sd, "bf16"
    dec.engine().set_graphs(1)


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def decoder160(request):
    dec, sd = _decoder(request.param, 160)
    yield dec, 160, sd, request.param
    dec.engine().set_graphs(1)


@pytest.fixture(scope="module")
def decoder_bf16():
    dec, sd = _decoder("bf16", 160)
    yield dec, 160, sd, "bf16"
    dec.engine().set_graphs(1)


def _inputs(T, lens, c_cond):
    """CPU tensors: mu, mask, spks (or None), z = randn * 0.667, x1 = randn, keep bool [B,T]"""
    g = torch.Generator().manual_seed(T)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()[:, None]
    mu = torch.randn(len(lens), 80, T, generator=g) * mask
    spks = torch.randn(len(lens), 64, generator=g) if c_cond == 224 else None
    z = torch.randn(len(lens), 80, T, generator=g) * 0.667
    x1 = torch.randn(len(lens), 80, T, generator=torch.Generator().manual_seed(1000 + T))
    keep = torch.zeros(len(lens), T, dtype=torch.bool)
    keep[0, 8:20] = True
    keep[1, :] = True
    keep[2, :5] = True
    keep[2, 12:] = True
    return mu, mask, spks, z, x1, keep


def _dev(v):
    return None if v is None else v.to(DEV)


def _row(v, b):
    return None if v is None else v[b:b + 1]


def _row_grids():
    from matcha_hip import runtime as rt
    return [rt.cosine_grid(3), torch.linspace(0, 1, 6), torch.tensor([0.0, 1.0]), rt.cosine_grid(3)]


def _times(which, b):
    """row b's (t_i, dt_i, t_{i+1}) as fp32 0-d tensors: the reference grid (formed in double, rounded once; dt = 1 / n)
    or an explicit one (dt = t[i + 1] - t[i] in fp32, t_{i+1} the grid value itself)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    if which == "counts":
        n = COUNTS[b]
        return [(f(i / n), f(1.0 / n), f((i + 1) / n)) for i in range(n)]
    g = _row_grids()[b].to(torch.float32)
    return [(g[i], g[i + 1] - g[i], g[i + 1]) for i in range(g.numel() - 1)]


def _path(z0, x1, tv):
    """p(t) in fp32; p(1) is x1 itself"""
    if float(tv) == 1.0:
        return x1
    return (1 - (1 - SIGMA) * tv) * z0 + tv * x1


def _loop(sd, mu, mask, z, spks, times, solver, x1=None, keep=None):
    """The solver loop of model.py:1086-1104 on one row; with x1 / keep the kept valid frames are clamped to the path
    before evaluation 0, after an Euler update and after both midpoint evaluations (the half-step input at t + dt/2)."""
    from oracle import matcha_oracle as O
    z0 = z
    sel = None if keep is None else (keep[:, None, :] & (mask != 0))
    clamp = (lambda v, tv: v) if sel is None else (lambda v, tv: torch.where(sel, _path(z0, x1, tv), v))
    z = clamp(z, times[0][0])
    for ti, dt, tn in times:
        pred = O.decoder_forward(sd, z, mask, mu, ti.expand(1), spks)
        if solver == "euler":
            z = clamp(z + pred * dt, tn)
        else:
            th = ti + dt * 0.5
            pm = O.decoder_forward(sd, clamp(z + pred * dt * 0.5, th), mask, mu, th.expand(1), spks)
            z = clamp(z + pm * dt, tn)
    return z


def _oracle(sd, c_cond, T, lens, solver, which, infill):
    key = (which, c_cond, T, solver, infill)
    if key not in _REFS:
        mu, mask, spks, z, x1, keep = _inputs(T, lens, c_cond)
        _REFS[key] = torch.cat([
            _loop(sd, _row(mu, b), _row(mask, b), _row(z, b), _row(spks, b), _times(which, b), solver,
                  _row(x1, b) if infill else None, _row(keep, b) if infill else None) for b in range(len(lens))])
    return _REFS[key]


def _free(keep, mask, b):
    return (~keep[b]) & (mask[b, 0] != 0)


# ---------------------------------------------------------------- 1. parity with the oracle loop
def _parity(decoder, case, solver):
    """fp32: max |d| < 2e-4 per row (test_gpu_solve_rows._check_rows' bound). bf16: rel-RMS over the free valid frames
    of the batch < 1e-2, and per row <= max(1e-2, 1.5 e_b), e_b the same row's error of the bf16 solve without infill
    against its own oracle loop (that file's rule). First, on the CPU references alone: infill moves the free frames
    of rows 0 and 2 by more than 10x the fp32 bound, so ignoring keep cannot pass; row 3 (nothing kept) is unmoved.
    Row 2 takes one step: under Euler its only evaluation reads p(t_0 = 0) = z0, so its free frames cannot move (0
    exactly) and what shows its keep is the kept frames themselves; under midpoint the second evaluation reads
    p(1/2) and they do move."""
    dec, c_cond, sd, prec = decoder
    T, lens = case
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    mu, mask, spks, z, x1, keep = _inputs(T, lens, c_cond)
    args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
    kw = dict(solver=solver, max_valid=max(lens))
    for which, n, span in (("counts", COUNTS, None), ("grids", None, _row_grids())):
        ref = _oracle(sd, c_cond, T, lens, solver, which, True)
        plain_ref = _oracle(sd, c_cond, T, lens, solver, which, False)
        for b in (0, 2):
            moved = (ref[b] - plain_ref[b])[:, _free(keep, mask, b)].abs().max().item()
            print(f"{which} T={T} {solver}: oracle row {b} free frames moved by {moved:.3f}")
            if b == 2 and solver == "euler":
                assert moved == 0.0, moved
                kv = keep[b] & (mask[b, 0] != 0)
                assert (ref[b] - plain_ref[b])[:, kv].abs().max().item() > 10 * 2e-4
            else:
                assert moved > 10 * 2e-4, (b, moved)
        assert torch.equal(ref[3], plain_ref[3])
        out = eng.solve(*args, n, t_span=span, x1=_dev(x1), keep=_dev(keep), sigma_min=SIGMA, **kw).cpu()
        assert torch.isfinite(out).all()
        tag = f"infill {which} T={T} {solver} c_cond={c_cond}"
        if prec == "fp32":
            errs = [(out[b] - ref[b]).abs().max().item() for b in range(4)]
            print(f"{tag}: fp32 max|d| per row {['%.2e' % e for e in errs]}")
            assert max(errs) < 2e-4, errs
            continue
        plain = eng.solve(*args, n, t_span=span, **kw).cpu()
        free = torch.stack([_free(keep, mask, b) for b in range(4)])[:, None].expand_as(out)
        whole = rel_rms(out[free], ref[free])
        rows = {b: rel_rms(out[b][:, _free(keep, mask, b)], ref[b][:, _free(keep, mask, b)]) for b in (0, 2, 3)}
        base = {b: rel_rms(plain[b], plain_ref[b]) for b in (0, 2, 3)}  # row 1 has no free frame
        print(f"{tag}: bf16 rel-RMS over free valid frames: batch {whole:.3e}, rows "
              f"{ {b: '%.2e' % e for b, e in rows.items()} }, without infill { {b: '%.2e' % e for b, e in base.items()} }")
        assert whole < 1e-2, whole
        for b, e in rows.items():
            assert e <= max(1e-2, 1.5 * base[b]), (b, e, base[b])


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_infill_matches_the_oracle_loop(decoder160, case, solver):
    _parity(decoder160, case, solver)


def test_infill_matches_the_oracle_loop_speaker_conditioned(decoder_bf16_spk):
    """c_cond = 224: the estimator-input slot's leading dimension is 256, the z columns still 0 .. 79"""
    _parity(decoder_bf16_spk, CASES[1], "euler")


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("solver", SOLVERS)
def test_kept_frames_are_x1_and_nothing_kept_is_the_plain_solve(decoder160, solver):
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder160
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    eng.set_graphs(1)
    seeds = torch.tensor([11, -5, 2 ** 40, 3], dtype=torch.int64, device=DEV)
    for T, lens in CASES:
        mu, mask, spks, z, x1, keep = (_dev(v) for v in _inputs(T, lens, c_cond))
        kw = dict(solver=solver, max_valid=max(lens))
        inf = dict(x1=x1, keep=keep, sigma_min=SIGMA)
        plain = eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, **kw)
        a = eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, **kw, **inf)
        valid = (mask != 0).expand_as(a)
        kept = keep[:, None, :].expand_as(a)
        # kept valid frames: the caller's bits; kept frames in the padding: what the plain solve leaves there
        assert torch.equal(a[kept & valid], x1[kept & valid])
        assert torch.equal(a[kept & ~valid], plain[kept & ~valid])
        assert torch.equal(a[~valid], plain[~valid])
        assert not torch.equal(a[0], plain[0]) and not torch.equal(a[2], plain[2])
        # row 3, nothing kept: the same bits with and without infill in the same call geometry
        assert torch.equal(a[3], plain[3])
        # explicit grids end at 1 too; keep as [B,1,T] floats
        g = eng.solve(pk, z, 0.8, mu, mask, spks, None, t_span=_row_grids(), x1=x1, keep=keep[:, None].float() * 3, **kw)
        assert torch.equal(g[kept & valid], x1[kept & valid])
        # nothing kept anywhere: the rows-path solve, and with one shared count the graph-replayed solve
        none = torch.zeros_like(keep)
        assert torch.equal(eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, x1=x1, keep=none, **kw), plain)
        assert torch.equal(eng.solve(pk, z, 0.8, mu, mask, spks, 3, x1=x1, keep=none, **kw),
                           eng.solve(pk, z, 0.8, mu, mask, spks, 3, **kw))
        # one shared count with kept frames
        s3 = eng.solve(pk, z, 0.8, mu, mask, spks, 3, **kw, **inf)
        assert torch.equal(s3[kept & valid], x1[kept & valid]) and torch.isfinite(s3).all()
        # deterministic; out may be the noise tensor itself
        assert torch.equal(eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, **kw, **inf), a)
        zc = z.clone()
        assert eng.solve(pk, zc, 0.8, mu, mask, spks, COUNTS, out=zc, **kw, **inf) is zc and torch.equal(zc, a)
        # seeded is the solve on seeded_noise: z0 of the path is the same stream
        s1 = eng.solve(pk, None, 0.667, mu, mask, spks, COUNTS, seeds=seeds, **kw, **inf)
        s2 = eng.solve(pk, rt.seeded_noise(seeds, T), 0.667, mu, mask, spks, COUNTS, **kw, **inf)
        assert torch.isfinite(s1).all() and torch.equal(s1, s2), (T, (s1 - s2).abs().max().item())
        assert torch.equal(s1[kept & valid], x1[kept & valid])
        # sorted counts (no gather, no scatter) are the same solve as the rows permuted
        order = sorted(range(4), key=lambda b: -COUNTS[b])
        perm = torch.tensor(order, device=DEV)
        srt = eng.solve(pk, z[perm], 0.8, mu[perm], mask[perm], None if spks is None else spks[perm],
                        [COUNTS[b] for b in order], x1=x1[perm], keep=keep[perm], sigma_min=SIGMA, **kw)
        assert torch.equal(srt, a[perm])


@pytest.mark.parametrize("solver", SOLVERS)
def test_infill_identical_under_kernel_variants(decoder_bf16, solver):
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder_bf16
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    for T, lens in CASES:
        mu, mask, spks, z, x1, keep = (_dev(v) for v in _inputs(T, lens, c_cond))
        outs = {}
        for km in (0, 1, 3, 15):
            prev = rt.set_decoder_kernels(km)
            try:
                outs[km] = eng.solve(pk, z, 1.0, mu, mask, spks, COUNTS, solver=solver, max_valid=max(lens), x1=x1,
                                     keep=keep).cpu()
            finally:
                rt.set_decoder_kernels(prev)
        for km in (1, 3, 15):
            assert torch.equal(outs[km], outs[0]), (T, km, (outs[km] - outs[0]).abs().max().item())


# ---------------------------------------------------------------- 3. the launch log
def test_one_clamp_launch_per_evaluation_on_the_rows_left(decoder_bf16):
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder_bf16
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    plan = rt.rows_plan(sorted(COUNTS, reverse=True))
    assert [4] + plan == [4, 4, 3, 3, 1, 1]
    for T, lens in CASES:
        mu, mask, spks, z, x1, keep = (_dev(v) for v in _inputs(T, lens, c_cond))
        logs = {}
        for name, inf in (("infill", dict(x1=x1, keep=keep)), ("plain", {})):
            rt.vconv_log_start(20000)
            try:
                eng.solve(pk, z, 1.0, mu, mask, spks, COUNTS, max_valid=max(lens), **inf)
                torch.cuda.synchronize()
            finally:
                logs[name] = rt.vconv_log_stop(20000)
        clamps = [r for r in logs["infill"] if r["ef"] == rt.INFILL_LOG]
        assert [r["B"] for r in clamps] == [4] + plan and all(r["L"] == T for r in clamps)
        assert [r["B"] for r in logs["infill"] if r["ef"] == rt.PROJ_LOG] == plan
        assert not [r for r in logs["plain"] if r["ef"] == rt.INFILL_LOG]
        assert len(logs["infill"]) == len(logs["plain"]) + 1 + len(plan)
    mu, mask, spks, z, x1, keep = (_dev(v) for v in _inputs(*CASES[0], c_cond))
    rt.vconv_log_start(20000)
    try:
        eng.solve(pk, z, 1.0, mu, mask, spks, COUNTS, solver="midpoint", max_valid=48, x1=x1, keep=keep)
        torch.cuda.synchronize()
    finally:
        log = rt.vconv_log_stop(20000)
    assert [r["B"] for r in log if r["ef"] == rt.INFILL_LOG] == [4] + rt.rows_plan(sorted(COUNTS, reverse=True),
                                                                                   "midpoint")


# ---------------------------------------------------------------- 4. synthesize end to end
def _lj_model():
    g = golden("g6_synth_lj")
    sd = weights_from(g)
    sd["encoder.proj_w.proj.weight"] = t(g["proj_w_weight"])
    sd["encoder.proj_w.proj.bias"] = t(g["proj_w_bias"])
    m = make_matcha(1, "fp32")
    m.load_state_dict(sd)
    return m.to(DEV).eval(), t(g["x"]).to(DEV), t(g["x_lengths"]).to(DEV)


def test_synthesize_infill_end_to_end_fp32():
    """kept frames come back within 1e-5: normalize, the solve's exact x1, denormalize are three fp32 roundings on
    values below 16, where an ulp is 9.5e-7"""
    m, x, xl = _lj_model()
    m.mel_mean.fill_(-5.5)
    m.mel_std.fill_(2.1)
    seeds = [7, -3]
    mel0, yl0, attn0 = m.synthesize(x, xl, n_timesteps=3, seeds=seeds)
    y_max = mel0.shape[-1]
    lens = yl0.tolist()
    assert min(lens) >= 12
    g = torch.Generator().manual_seed(5)
    want = (torch.randn(2, 80, y_max + 7, generator=g) * 2.1 - 5.5).clamp(-15.9, 15.9).to(DEV)
    keep = torch.zeros(2, y_max + 7, dtype=torch.bool, device=DEV)
    keep[0, 3:lens[0] // 2] = True
    keep[1, 2:9] = True
    keep[1, lens[1] - 4:] = True  # to the end of the buffer: past y_lengths[1] it is ignored

    def check(mel, tk):
        assert mel.shape == mel0.shape and torch.isfinite(mel).all()
        for b in range(2):
            k = torch.zeros(y_max, dtype=torch.bool, device=DEV)  # kept, given (< tk) and valid (< y_lengths[b])
            k[:min(tk, y_max)] = keep[b, :min(tk, y_max)]
            k[lens[b]:] = False
            assert k.any()
            err = (mel[b][:, k] - want[b, :, :y_max][:, k]).abs().max().item()
            print(f"synthesize infill Tk={tk} row {b}: kept frames max|d| {err:.2e}")
            assert err <= 1e-5, (b, tk, err)
            free = ~k
            free[lens[b]:] = False
            assert not torch.equal(mel[b][:, free], mel0[b][:, free])  # the free frames see the kept ones

    for tk in (y_max + 7, y_max, y_max - 5):  # longer than t_pad may be (cropped), exact, shorter (the tail is free)
        mel, yl, attn = m.synthesize(x, xl, n_timesteps=3, seeds=seeds, infill_mel=want[:, :, :tk],
                                     infill_keep=keep[:, :tk])
        assert torch.equal(yl, yl0) and torch.equal(attn, attn0)
        check(mel, tk)
    out = m.synthesise(x, xl, 3, seeds=seeds, infill_mel=want[:, :, :y_max - 5], infill_keep=keep[:, :y_max - 5])
    assert torch.equal(out["mel"], mel) and torch.equal(out["mel_lengths"], yl0)
    # per-utterance counts go through the same call
    mel_c, yl_c, _ = m.synthesize(x, xl, n_timesteps=[2, 3], seeds=seeds, infill_mel=want, infill_keep=keep)
    assert torch.equal(yl_c, yl0)
    check(mel_c, y_max + 7)


# ---------------------------------------------------------------- 5. edit
def test_edit_keeps_the_frames_outside_the_span_fp32():
    m, x_old, xl_old = _lj_model()
    B, Tx = x_old.shape
    lo = xl_old.tolist()
    assert min(lo) >= 9
    starts = [2, 4]
    new_ids = torch.tensor([[31, 32, 33, 34, 35], [41, 42, 43, 44, 45]], device=DEV)
    x_new = torch.zeros(B, Tx + 2, dtype=x_old.dtype, device=DEV)
    spans = []
    for b, a in enumerate(starts):  # 3 tokens [a, a + 3) replaced by 5
        x_new[b, :a] = x_old[b, :a]
        x_new[b, a:a + 5] = new_ids[b]
        x_new[b, a + 5:lo[b] + 2] = x_old[b, a + 3:lo[b]]
        spans.append((a, a + 3, a + 5))
    xl_new = xl_old + 2
    d = torch.zeros(B, Tx, dtype=torch.int64, device=DEV)  # planted durations: 2, 3, 4, 2, ... frames per token
    for b in range(B):
        d[b, :lo[b]] = 2 + torch.arange(lo[b], device=DEV) % 3
    seeds = [7, -3]
    A, yl_a, _ = m.synthesize(x_old, xl_old, 3, durations=d, seeds=seeds)
    assert torch.equal(yl_a, d.sum(1))
    d_pred = m.predict_durations(x_new, xl_new)
    d_new = torch.zeros(B, Tx + 2, dtype=torch.int64, device=DEV)
    for b, a in enumerate(starts):
        d_new[b, :a] = d[b, :a]
        d_new[b, a:a + 5] = d_pred[b, a:a + 5]
        d_new[b, a + 5:lo[b] + 2] = d[b, a + 3:lo[b]]
    for margin in (0, 2):
        mel, yl, keep = m.edit(x_old, xl_old, A, yl_a, x_new, xl_new, spans, 3, durations_old=d, margin=margin,
                               seeds=seeds)
        assert torch.equal(yl, d_new.sum(1)) and mel.shape[-1] == int(yl.max()) and keep.shape == (B, mel.shape[-1])
        assert keep.dtype == torch.bool and torch.isfinite(mel).all()
        for b, a in enumerate(starts):
            f_a, f_b = int(d[b, :a].sum()), int(d[b, :a + 3].sum())
            g_b, y_new = int(d_new[b, :a + 5].sum()), int(yl[b])
            assert y_new - g_b == int(yl_a[b]) - f_b
            want_keep = torch.zeros(mel.shape[-1], dtype=torch.bool, device=DEV)
            want_keep[:max(f_a - margin, 0)] = True
            want_keep[g_b + margin:y_new] = True
            assert torch.equal(keep[b], want_keep), (b, margin)
            assert not keep[b, f_a:g_b].any()
            pre = (mel[b, :, :f_a - margin] - A[b, :, :f_a - margin]).abs().max().item()
            tail = (mel[b, :, g_b + margin:y_new] - A[b, :, f_b + margin:int(yl_a[b])]).abs().max().item()
            print(f"edit margin {margin} row {b}: prefix max|d| {pre:.2e}, tail max|d| {tail:.2e}")
            assert pre <= 1e-5 and tail <= 1e-5, (b, margin, pre, tail)
    # a no-op span returns the recording
    mel, yl, keep = m.edit(x_old, xl_old, A, yl_a, x_old, xl_old, [(3, 3, 3), (5, 5, 5)], 3, durations_old=d,
                           seeds=seeds)
    assert torch.equal(yl, yl_a)
    for b in range(B):
        assert keep[b, :int(yl[b])].all()
        assert (mel[b, :, :int(yl[b])] - A[b, :, :int(yl[b])]).abs().max().item() <= 1e-5
    # without durations_old the aligner supplies them: the lengths are consistent with its durations
    d_al = m.align(x_old, xl_old, A, yl_a)
    mel, yl, keep = m.edit(x_old, xl_old, A, yl_a, x_new, xl_new, spans, 3, seeds=seeds)
    want = [int(d_al[b, :a].sum() + d_pred[b, a:a + 5].sum() + d_al[b, a + 3:lo[b]].sum()) for b, a in enumerate(starts)]
    assert yl.tolist() == want and torch.isfinite(mel).all() and keep.shape == (B, mel.shape[-1])
