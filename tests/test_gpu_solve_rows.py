"""Per-utterance step counts and time grids in one CFM solve (MI355X, mt_cfm_solve_rows): every row against the CPU
oracle's solve of that row alone, explicit grids against a reference loop over the oracle's estimator, the exact
identities (scalar path untouched, seeds, kernel variants), the launch log (rows really leave the batch after their
last step), synthesize end to end, and the argument errors.

Counts in caller order [3, 5, 1, 3]: unsorted, a tie, a one-step row; sorted [5, 3, 3, 1] the Euler evaluations run on
4, 3, 3, 1, 1 rows. T = 48 has an unpadded row (general attention), T = 108 pads every row at both U-Net levels (with
max_valid the bf16 solver takes the query-independent attention path)."""
import numpy as np
import pytest
import torch

from conftest import HP, golden, make_decoder, make_matcha, rel_rms, t, weights_from

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = [3, 5, 1, 3]
CASES = [(48, [48, 30, 17, 40]), (108, [105, 76, 46, 90])]
CASE_IDS = ["T48-general", "T108-uniform"]
SOLVERS = ["euler", "midpoint"]

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


@pytest.fixture(scope="module", params=[("fp32", 160), ("bf16", 160), ("fp32", 224), ("bf16", 224)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def decoder(request):
    prec, c_cond = request.param
    dec, sd = _decoder(prec, c_cond)
    yield dec, c_cond, sd, prec
    dec.engine().set_graphs(1)


@pytest.fixture(scope="module")
def decoder_bf16():
    dec, sd = _decoder("bf16", 160)
    yield dec, 160, sd, "bf16"
    dec.engine().set_graphs(1)


def _inputs(T, lens, c_cond):
    """CPU tensors: mu, mask, spks (or None), z = randn * 0.667"""
    g = torch.Generator().manual_seed(T)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()[:, None]
    mu = torch.randn(len(lens), 80, T, generator=g) * mask
    spks = torch.randn(len(lens), 64, generator=g) if c_cond == 224 else None
    z = torch.randn(len(lens), 80, T, generator=g) * 0.667
    return mu, mask, spks, z


def _dev(v):
    return None if v is None else v.to(DEV)


def _row(v, b):
    return None if v is None else v[b:b + 1]


def _oracle_counts(sd, c_cond, T, lens, solver):
    """row b: the oracle's n_b-step solve of that row alone -> [B,80,T]"""
    from oracle import matcha_oracle as O
    key = ("counts", c_cond, T, solver)
    if key not in _REFS:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        _REFS[key] = torch.cat([
            O.cfm_solve(sd, _row(mu, b), _row(mask, b), COUNTS[b], _row(z, b), _row(spks, b), solver)
            for b in range(len(lens))])
    return _REFS[key]


def _grid_loop(sd, mu, mask, z, spks, grid, solver):
    """The solver loop of model.py:1086-1104 on an explicit fp32 grid: dt = t[i + 1] - t[i] in fp32."""
    from oracle import matcha_oracle as O
    grid = grid.to(torch.float32)
    b = z.shape[0]
    for i in range(grid.numel() - 1):
        ti = grid[i].expand(b)
        dt = grid[i + 1] - grid[i]
        pred = O.decoder_forward(sd, z, mask, mu, ti, spks)
        if solver == "euler":
            z = z + pred * dt
        else:
            pm = O.decoder_forward(sd, z + pred * dt * 0.5, mask, mu, ti + dt * 0.5, spks)
            z = z + pm * dt
    return z


def _row_grids():
    from matcha_hip import runtime as rt
    return [rt.cosine_grid(3), torch.linspace(0, 1, 6), torch.tensor([0.0, 1.0]), rt.cosine_grid(3)]


def _oracle_grids(sd, c_cond, T, lens, solver, which):
    from matcha_hip import runtime as rt
    key = (which, c_cond, T, solver)
    if key not in _REFS:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        if which == "shared":
            _REFS[key] = _grid_loop(sd, mu, mask, z, spks, rt.cosine_grid(4), solver)
        else:
            _REFS[key] = torch.cat([_grid_loop(sd, _row(mu, b), _row(mask, b), _row(z, b), _row(spks, b), g, solver)
                                    for b, g in enumerate(_row_grids())])
    return _REFS[key]


def _check_rows(tag, prec, out, ref, counts, uniform_solve):
    """fp32: every row within test_cfm_solver_fp32's bound of its reference. bf16: the whole batch within SURVEY §8c's
    rel-RMS 1e-2, and row b within max(1e-2, 1.5 e_b), e_b the error on that row (against the oracle's n_b-step
    solve of the row alone) of the existing shared-count n_b-step bf16 solve of the whole batch: the two paths round
    the same quantities the same number of times, apart from the GroupNorm partial-sum order at a smaller batch."""
    if prec == "fp32":
        errs = [(out[b] - ref[b]).abs().max().item() for b in range(len(counts))]
        print(f"{tag}: fp32 max|d| per row {['%.2e' % e for e in errs]}")
        assert max(errs) < 2e-4, errs
        return
    whole = rel_rms(out, ref)
    rows = [rel_rms(out[b], ref[b]) for b in range(len(counts))]
    base = [rel_rms(uniform_solve(counts[b])[b], ref[b]) if uniform_solve else None for b in range(len(counts))]
    print(f"{tag}: bf16 rel-RMS batch {whole:.3e}, rows {['%.2e' % e for e in rows]}, "
          f"shared-count rows {['-' if e is None else '%.2e' % e for e in base]}")
    assert whole < 1e-2, whole
    for b, e in enumerate(rows):
        assert e <= max(1e-2, 1.5 * (base[b] or 0.0)), (b, e, base[b])


# ---------------------------------------------------------------- 1. counts against the oracle, per row
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_mixed_counts_match_the_oracle_per_row(decoder, case, solver):
    dec, c_cond, sd, prec = decoder
    T, lens = case
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    mu, mask, spks, z = _inputs(T, lens, c_cond)
    ref = _oracle_counts(sd, c_cond, T, lens, solver)
    args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
    kw = dict(solver=solver, max_valid=max(lens))
    out = eng.solve(*args, COUNTS, **kw).cpu()
    assert torch.isfinite(out).all()
    uni = {}

    def uniform_solve(n):  # the oracle references of the rows with n steps double as the shared-count solve's
        if n not in uni:
            uni[n] = eng.solve(*args, n, **kw).cpu()
        return uni[n]

    _check_rows(f"counts T={T} {solver} c_cond={c_cond}", prec, out, ref, COUNTS, uniform_solve)
    # a row with more steps is not the row with fewer: the counts really are per row
    assert not torch.equal(out[0], uniform_solve(5)[0])


# ---------------------------------------------------------------- 2. explicit grids
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_t_span_matches_the_reference_loop(decoder, case, solver):
    """One cosine grid shared by the batch, and one grid per row (cosine 3, uniform 5, one step, cosine 3). The bf16
    rows' e_b is that of the shared-count solve with the grid's number of steps (the same number of bf16 roundings;
    its reference the oracle's solve on the reference grid)."""
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder
    T, lens = case
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    mu, mask, spks, z = _inputs(T, lens, c_cond)
    args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
    kw = dict(solver=solver, max_valid=max(lens))
    counts_ref = _oracle_counts(sd, c_cond, T, lens, solver)
    uni = {}

    def base_error(n, b):
        from oracle import matcha_oracle as O
        if n not in uni:
            uni[n] = eng.solve(*args, n, **kw).cpu()
        if n == COUNTS[b]:
            return rel_rms(uni[n][b], counts_ref[b])
        key = ("uniform", c_cond, T, solver, n, b)
        if key not in _REFS:
            _REFS[key] = O.cfm_solve(sd, _row(mu, b), _row(mask, b), n, _row(z, b), _row(spks, b), solver)[0]
        return rel_rms(uni[n][b], _REFS[key])

    for which, span, counts in (("shared", rt.cosine_grid(4), [4] * 4), ("per-row", _row_grids(), COUNTS)):
        ref = _oracle_grids(sd, c_cond, T, lens, solver, which)
        out = eng.solve(*args, None, t_span=span, **kw).cpu()
        assert torch.isfinite(out).all()
        tag = f"t_span {which} T={T} {solver} c_cond={c_cond}"
        if prec == "fp32":
            _check_rows(tag, prec, out, ref, counts, None)
        else:
            whole = rel_rms(out, ref)
            rows = [rel_rms(out[b], ref[b]) for b in range(4)]
            base = [base_error(counts[b], b) for b in range(4)]
            print(f"{tag}: bf16 rel-RMS batch {whole:.3e}, rows {['%.2e' % e for e in rows]}, "
                  f"shared-count rows {['%.2e' % e for e in base]}")
            assert whole < 1e-2, whole
            for b in range(4):
                assert rows[b] <= max(1e-2, 1.5 * base[b]), (b, rows[b], base[b])
        # the counts may come along, as long as they agree
        assert torch.equal(eng.solve(*args, counts, t_span=span, **kw).cpu(), out)
    # the reference's own grid given explicitly is not the reference path: dt = t[i + 1] - t[i], not 1 / n
    lin = eng.solve(*args, None, t_span=torch.linspace(0, 1, 4), **kw).cpu()
    assert torch.isfinite(lin).all() and lin.shape == z.shape


# ---------------------------------------------------------------- 3. exact identities
@pytest.mark.parametrize("solver", SOLVERS)
def test_equal_counts_take_the_scalar_path(decoder, solver):
    """B equal counts are the int: the graph-replayed solve, bit for bit (graphs on)"""
    dec, c_cond, sd, prec = decoder
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    eng.set_graphs(1)
    for T, lens in CASES:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
        kw = dict(solver=solver, max_valid=max(lens))
        a = eng.solve(*args, 3, **kw)
        assert torch.equal(eng.solve(*args, [3, 3, 3, 3], **kw), a)
        assert torch.equal(eng.solve(*args, torch.tensor([3, 3, 3, 3]), **kw), a)
        assert torch.equal(eng.solve(*args, torch.tensor([3, 3, 3, 3], device=DEV), **kw), a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_mixed_solve_is_deterministic_and_seeded(decoder, solver):
    """the same mixed call twice: the same bits; solve(seeds=...) mixed is the mixed solve on seeded_noise(...), for one
    shared temperature and for one per row; `out` may be the noise tensor itself (CFM.forward's out=z)"""
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    seeds = torch.tensor([11, -5, 2 ** 40, 3], dtype=torch.int64, device=DEV)
    tau_b = torch.tensor([0.667, 0.3, 1.0, 0.5], device=DEV)
    for T, lens in CASES:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        mu, mask, spks, z = _dev(mu), _dev(mask), _dev(spks), _dev(z)
        kw = dict(solver=solver, max_valid=max(lens))
        a = eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, **kw)
        assert torch.equal(eng.solve(pk, z, 0.8, mu, mask, spks, COUNTS, **kw), a)
        zc = z.clone()
        assert eng.solve(pk, zc, 0.8, mu, mask, spks, COUNTS, out=zc, **kw) is zc and torch.equal(zc, a)
        s1 = eng.solve(pk, None, 0.667, mu, mask, spks, COUNTS, seeds=seeds, **kw)
        s2 = eng.solve(pk, rt.seeded_noise(seeds, T), 0.667, mu, mask, spks, COUNTS, **kw)
        assert torch.isfinite(s1).all() and torch.equal(s1, s2), (T, (s1 - s2).abs().max().item())
        p1 = eng.solve(pk, None, tau_b, mu, mask, spks, COUNTS, seeds=seeds, **kw)
        p2 = eng.solve(pk, rt.seeded_noise(seeds, T, temperature=tau_b), 1.0, mu, mask, spks, COUNTS, **kw)
        assert torch.equal(p1, p2), (T, (p1 - p2).abs().max().item())
        assert not torch.equal(s1, p1)
        # sorted counts (no gather, no scatter) are the same solve as the rows permuted
        order = sorted(range(4), key=lambda b: -COUNTS[b])
        perm = torch.tensor(order, device=DEV)
        srt = eng.solve(pk, z[perm], 0.8, mu[perm], mask[perm], None if spks is None else spks[perm],
                        [COUNTS[b] for b in order], **kw)
        assert torch.equal(srt, a[perm])


@pytest.mark.parametrize("solver", SOLVERS)
def test_mixed_solve_identical_under_kernel_variants(decoder_bf16, solver):
    """mt_decoder_set_kernels' contract on the new path: masks 0, 1, 3 and 15 give the same bits (the dedicated final
    projection kernel against the generic epilogue, both reading one dt per utterance; the cached o_b over shrinking
    batches; the store policies)"""
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder_bf16
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    for T, lens in CASES:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
        outs = {}
        for km in (0, 1, 3, 15):
            prev = rt.set_decoder_kernels(km)
            try:
                outs[km] = eng.solve(*args, COUNTS, solver=solver, max_valid=max(lens)).cpu()
            finally:
                rt.set_decoder_kernels(prev)
        for km in (1, 3, 15):
            assert torch.equal(outs[km], outs[0]), (T, km, (outs[km] - outs[0]).abs().max().item())


# ---------------------------------------------------------------- 4. rows really retire
def test_rows_leave_the_batch_after_their_last_step(decoder_bf16):
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder_bf16
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    plan = rt.rows_plan(sorted(COUNTS, reverse=True))
    assert plan == [4, 3, 3, 1, 1]
    for T, lens in CASES:
        mu, mask, spks, z = _inputs(T, lens, c_cond)
        rt.vconv_log_start(20000)
        try:
            eng.solve(pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks), COUNTS, max_valid=max(lens))
            torch.cuda.synchronize()
        finally:
            log = rt.vconv_log_stop(20000)
        assert [r["B"] for r in log if r["ef"] == rt.PROJ_LOG] == plan
        ev = 0  # the evaluation a record belongs to: its final projection closes it
        for r in log:
            assert ev < len(plan) and r["B"] <= plan[ev], (ev, r)
            ev += r["ef"] == rt.PROJ_LOG
        assert ev == len(plan) and len(log) > 10 * len(plan)


# ---------------------------------------------------------------- 5. end to end
def test_synthesize_mixed_counts_end_to_end_fp32():
    from matcha_hip.noise import reference_noise
    from oracle import matcha_oracle as O
    g = golden("g6_synth_lj")
    sd = weights_from(g)
    sd["encoder.proj_w.proj.weight"] = t(g["proj_w_weight"])
    sd["encoder.proj_w.proj.bias"] = t(g["proj_w_bias"])
    m = make_matcha(1, "fp32")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x, xl = t(g["x"]), t(g["x_lengths"])
    counts, seeds = [2, 4], [7, -3]
    mel, yl, attn = m.synthesize(x.to(DEV), xl.to(DEV), n_timesteps=counts, seeds=seeds)
    mel_s, yl_s, attn_s = m.synthesize(x.to(DEV), xl.to(DEV), n_timesteps=4, seeds=seeds)
    assert torch.equal(yl, yl_s) and torch.equal(attn, attn_s)
    assert (mel[1] - mel_s[1]).abs().max() < 2e-4  # row 1 takes 4 steps in both
    hp = dict(HP, n_spks=1)
    mu, logw, x_mask = O.text_encoder(O.sub(sd, "encoder"), x, xl, hp, None)
    yl_o, y_max, t_pad, y_mask, attn_o, mu_y = O.align(logw, x_mask, mu, 1.0)
    assert torch.equal(yl.cpu(), yl_o) and torch.equal(attn.cpu(), attn_o)
    for b in range(2):
        z = torch.from_numpy(np.asarray(reference_noise(seeds[b], t_pad), dtype=np.float32))[None]
        ref = O.cfm_solve(O.sub(sd, "decoder.estimator"), mu_y[b:b + 1], y_mask[b:b + 1], counts[b], z, None, "euler")
        ref = O.denormalize(ref, sd["mel_mean"], sd["mel_std"])[0, :, :y_max]
        err = (mel[b].cpu() - ref).abs().max().item()
        print(f"row {b} ({counts[b]} steps): mel max|d| {err:.3e}")
        assert err < 2e-4, (b, err)
    out = m.synthesise(x.to(DEV), xl.to(DEV), torch.tensor(counts), seeds=seeds)
    assert torch.equal(out["mel"], mel) and torch.equal(out["mel_lengths"], yl)
    # a shared grid through the public interface: the reference's grid spelled out takes dt = t[i + 1] - t[i]
    mel_g, yl_g, _ = m.synthesize(x.to(DEV), xl.to(DEV), None, seeds=seeds, t_span=torch.linspace(0, 1, 5))
    assert torch.equal(yl_g, yl) and (mel_g - mel_s).abs().max() < 2e-4


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(decoder_bf16):
    from matcha_hip import runtime as rt
    dec, c_cond, sd, prec = decoder_bf16
    eng, pk = dec.engine(), dec.packed(torch.device(DEV))
    T, lens = CASES[0]
    mu, mask, spks, z = _inputs(T, lens, c_cond)
    args = (pk, _dev(z), 1.0, _dev(mu), _dev(mask), _dev(spks))
    for n, span in [([3, 5, 1], None),                              # wrong length
                    ([3, 5, 0, 3], None),                           # a count < 1
                    (3, rt.cosine_grid(4)),                         # t_span and a disagreeing n_timesteps
                    ([3, 5, 1, 3], [rt.cosine_grid(3)] * 4),
                    (None, [rt.cosine_grid(3)] * 3),                # three grids for four rows
                    (None, torch.tensor([0.0, 0.6, 0.5, 1.0])),     # not increasing
                    (None, torch.tensor([0.0, 0.5, 0.5, 1.0])),     # not strictly
                    (None, torch.tensor([0.0, 0.5, 1.25])),         # outside [0, 1]
                    (None, None)]:
        with pytest.raises(ValueError):
            eng.solve(*args, n, t_span=span)
    with pytest.raises(TypeError):  # one temperature per row still needs seeds, mixed or not
        eng.solve(pk, _dev(z), torch.ones(4), _dev(mu), _dev(mask), _dev(spks), COUNTS)
    m = make_matcha(1, "fp32").to(DEV).eval()
    x, xl = torch.randint(1, 178, (2, 9), device=DEV), torch.tensor([9, 7], device=DEV)
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=[2, 4, 2])
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=[2, 0])
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=2, t_span=rt.cosine_grid(3))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, n_timesteps=None, t_span=[0.0, 1.0, 0.5])
    # the C entry point takes sorted rows only and says so
    ws = torch.empty(rt.lib().mt_cfm_rows_workspace_bytes(eng.h, 4, T, 5, 0), dtype=torch.uint8, device=DEV)
    import ctypes
    n_bad = (ctypes.c_int32 * 4)(3, 5, 1, 3)
    out = torch.empty_like(args[1])
    rc = rt.lib().mt_cfm_solve_rows(eng.h, pk.data_ptr(), args[1].data_ptr(), None, None, args[3].data_ptr(),
                                    args[4].data_ptr(), None, 4, T, 0, n_bad, None, None, 0, out.data_ptr(),
                                    ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"sorted" in rt.lib().mt_last_error()
