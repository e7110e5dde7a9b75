"""Streamed level control, host side (CPU only: no kernel launches): the fixed-gain limiter's
specification (matcha_hip/limiter.py), the finality rules and the three ranges of the plan (matcha_hip/stream_plan.py),
a numpy run of the two range stages along a plan against the one-pass result, bit for bit, and every new refusal of
AudioOutput, WaveStreamer and the C ABI."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import make_generator

from matcha_hip import audio_out as ao
from matcha_hip import limiter as lm
from matcha_hip import stream_plan as sp

C_DB = -1.0
C32 = np.float32(10.0 ** (C_DB / 20.0))
POISON = np.float32(1e30)  # finite: a NaN counts as absent in the envelope and would hide a read
HALF4 = ao.design_filter(4, 1)[1]
EREACH = lm.envelope_reach(HALF4)


def _row(n, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


# ---- the specification -----------------------------------------------------------------------------------------

def test_fixed_gain_ref_is_its_definition():
    for db in (0.0, 6.0, -6.0, 20.0, 12.345, -80.0, 1e-3):
        g = lm.fixed_gain_ref(db)
        assert isinstance(g, np.float32) and g == np.float32(10.0 ** (np.float64(db) / 20.0))
    assert lm.fixed_gain_ref(0) == np.float32(1.0) and lm.fixed_gain_ref(20) == np.float32(10.0)
    assert lm.fixed_gain_ref(np.float32(6.0)) == lm.fixed_gain_ref(6.0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lm.fixed_gain_ref(bad)


@pytest.mark.parametrize("W", [1, 2, 80, 2048])
def test_limit_fixed_ref_is_its_definition(W):
    x = _row(3000, W)
    for db in (6.0, 20.0):
        y, red = lm.limit_fixed_ref(x, db, C_DB, W)
        g = lm.fixed_gain_ref(db)
        s = lm.gain_curve_ref(lm.envelope_ref(x), g, C32, W)
        assert y.dtype == np.float32 and np.array_equal(y, lm.apply_ref(x, g, s))
        assert red == s.min() and red < 1.0
        # every delivered sample's envelope is held at the ceiling, up to the product's rounding
        a = (g * lm.envelope_ref(x)).astype(np.float32)
        assert (a * s <= C32 * np.float32(1 + 2.0 ** -22)).all()
        assert (np.abs(y) <= C32 * np.float32(1 + 2.0 ** -22)).all()
    y, red = lm.limit_fixed_ref(np.zeros(0, np.float32), 6.0, C_DB, W)
    assert y.shape == (0,) and red == np.float32(1.0)
    # no "levelled at all" test: a silent row is g * 0
    y, red = lm.limit_fixed_ref(np.zeros(50, np.float32), 6.0, C_DB, W)
    assert np.array_equal(y, np.zeros(50, np.float32)) and red == np.float32(1.0)
    with pytest.raises(ValueError):
        lm.limit_fixed_ref(x, float("nan"), C_DB, W)


def burst_signal(fs=16000, seed=0):
    """DESIGN §23's signal: 2 s of noise of sigma 0.02 with twelve 8-sample bursts of sigma 0.5"""
    rng = np.random.default_rng(seed)
    n = 2 * fs
    x = rng.standard_normal(n) * 0.02
    for p in rng.choice(np.arange(200, n - 200, 400), 12, replace=False):
        x[p:p + 8] = rng.standard_normal(8) * 0.5
    return x.astype(np.float32)


def test_limit_fixed_ref_is_the_first_pass_of_limiter_ref():
    x = burst_signal()
    trace = []
    y1, g1, red1, _ = lm.limiter_ref(x, 16000, -16.0, C_DB, 80, passes=1, trace=trace)
    assert g1 == trace[0][0] and g1 > 1.0
    db = 20.0 * math.log10(float(g1))
    assert lm.fixed_gain_ref(db) == g1  # fp64 carries an fp32 gain through dB and back
    y, red = lm.limit_fixed_ref(x, db, C_DB, 80)
    assert np.array_equal(y, y1) and red == red1 and red < 1.0


@pytest.mark.parametrize("W", [1, 2, 80, 2048])
def test_gain_one_where_nothing_near_is_over_the_ceiling(W):
    x = _row(6000, 5, 0.02)
    x[3000:3004] = np.float32(0.9)
    db = 6.0
    g = lm.fixed_gain_ref(db)
    p = lm.envelope_ref(x)
    over = np.flatnonzero((g * p).astype(np.float32) > C32)
    assert over.size and over.min() >= 2990 and over.max() <= 3013
    s = lm.gain_curve_ref(p, g, C32, W)
    y, _ = lm.limit_fixed_ref(x, db, C_DB, W)
    i = np.arange(len(x))
    far = (i < over.min() - (W - 1)) | (i > over.max() + (W - 1))
    assert far.any() and (s[far] == 1.0).all() and (s[over] < 1.0).all()
    assert np.array_equal(y[far], (g * x).astype(np.float32)[far])
    if W > 1:  # and the window is used to its edge on both sides
        assert s[over.min() - (W - 1)] < 1.0 and s[over.max() + (W - 1)] < 1.0


# ---- reach and finality ----------------------------------------------------------------------------------------

def test_envelope_reach():
    assert HALF4 == 40 and EREACH == 10
    for half4 in (0, 1, 2, 4, 5, 40, 41, 1024):
        assert lm.envelope_reach(half4) == (half4 + 3) // 4
        # the chain of the 4x output 4 i + 3 starts at the sample (half4 + 4 i + 3) // 4
        for i in (0, 7, 1000):
            assert (half4 + 4 * i + 3) // 4 == i + lm.envelope_reach(half4)
    with pytest.raises(ValueError):
        lm.envelope_reach(-1)


def test_finality_functions():
    assert sp.envelope_final(100, 100, 10) == 100 and sp.envelope_final(101, 100, 10) == 100
    assert sp.envelope_final(99, 100, 10) == 89 and sp.envelope_final(10, 100, 10) == 0
    assert sp.envelope_final(3, 100, 10) == 0 and sp.envelope_final(0, 0, 10) == 0
    assert sp.limit_final(100, 100, 80) == 100 and sp.limit_final(99, 100, 80) == 20
    assert sp.limit_final(79, 100, 80) == 0 and sp.limit_final(5, 100, 80) == 0
    assert sp.limit_final(99, 100, 1) == 99 and sp.limit_final(0, 0, 2048) == 0


def test_envelope_final_is_tight():
    """p[:i + 1] needs x[:i + EREACH + 1], all of it: poisoning from i + 11 on changes nothing, from i + 10 on does"""
    x = _row(3000, 11)
    p = lm.envelope_ref(x)
    for i in (0, 1, 511, 1500, 2980):
        ok, bad = x.copy(), x.copy()
        ok[i + EREACH + 1:] = POISON
        bad[i + EREACH:] = POISON
        assert np.array_equal(lm.envelope_ref(ok)[:i + 1], p[:i + 1]), i
        assert not np.array_equal(lm.envelope_ref(bad)[:i + 1], p[:i + 1]), i
        assert sp.envelope_final(i + EREACH + 1, 3000, EREACH) == i + 1
    assert sp.envelope_final(3000, 3000, EREACH) == 3000


@pytest.mark.parametrize("W", [1, 2, 80, 2048])
def test_limit_final_is_tight(W):
    """s[:i + 1] needs p[:i + W], all of it"""
    x = _row(3000, 12)
    p = lm.envelope_ref(x)
    g = lm.fixed_gain_ref(12.0)
    s = lm.gain_curve_ref(p, g, C32, W)
    for i in (0, 300, 900):
        ok, bad = p.copy(), p.copy()
        ok[i + W:] = POISON
        bad[i + W - 1:] = POISON
        assert np.array_equal(lm.gain_curve_ref(ok, g, C32, W)[:i + 1], s[:i + 1]), i
        assert not np.array_equal(lm.gain_curve_ref(bad, g, C32, W)[:i + 1], s[:i + 1]), i
        if i + W < 3000:
            assert sp.limit_final(i + W, 3000, W) == i + 1


# ---- the plan ----------------------------------------------------------------------------------------------------

RATES = {8000: (160, 441), 16000: (320, 441), 22050: (1, 1), 48000: (320, 147)}


def _half(up, down):
    return 0 if (up, down) == (1, 1) else ao.design_filter(up, down)[1]


@pytest.mark.parametrize("rate", sorted(RATES))
@pytest.mark.parametrize("W", [1, 80, 2048])
@pytest.mark.parametrize("chunk,first", [(1, None), (5, None), (16, 8), (32, 4)])
def test_plan_ranges(rate, W, chunk, first):
    up, down = RATES[rate]
    assert ao.rates(22050, rate) == (up, down)
    half = _half(up, down)
    rng = np.random.RandomState(rate // 50 + W + chunk)
    lens = [0, 1] + [int(v) for v in rng.randint(2, 90, size=5)]
    rng.shuffle(lens)
    B = len(lens)
    pl = sp.plan(lens, chunk, first, up, down, half, reach=13, env_reach=EREACH, window=W)
    old = sp.plan(lens, chunk, first, up, down, half, reach=13)
    assert pl.env_reach == EREACH and pl.window == W and old.env_reach is None and old.window is None
    assert len(pl.steps) == len(old.steps) and pl.n_out == old.n_out
    y_done, done_count = [0] * B, [0] * B
    prev = None
    for st, so in zip(pl.steps, old.steps):
        # the stages before the limiter are the plan without one
        assert (st.s, st.e, st.m_lo, st.m_hi, st.raw_final, st.den_final, st.out_final) == \
               (so.s, so.e, so.m_lo, so.m_hi, so.raw_final, so.den_final, so.out_final)
        assert (so.p_lo, so.p_hi, so.y_lo, so.y_hi) == (None,) * 4 and so.delivered == (so.m_lo, so.m_hi)
        # each of the three ranges continues the one before it, in order
        for lo, hi, name in ((st.m_lo, st.m_hi, "m_hi"), (st.p_lo, st.p_hi, "p_hi"), (st.y_lo, st.y_hi, "y_hi")):
            assert lo == (getattr(prev, name) if prev else 0) and hi >= lo
        assert st.y_hi <= st.p_hi <= st.m_hi and st.delivered == (st.y_lo, st.y_hi)
        for b, n in enumerate(pl.n_out):
            if st.den_final[b] < lens[b]:  # an open row: what it reads is final
                assert min(st.m_hi, n) <= st.out_final[b]
                assert st.p_hi <= sp.envelope_final(st.m_hi, n, EREACH)
                assert st.y_hi <= sp.limit_final(st.p_hi, n, W)
            # and for every row, clipped to its own count, open or not
            assert min(st.p_hi, n) <= sp.envelope_final(min(st.m_hi, n), n, EREACH)
            assert min(st.y_hi, n) <= sp.limit_final(min(st.p_hi, n), n, W)
        for b, (off, cnt, done) in enumerate(st.out_counts(pl.n_out)):
            assert off == y_done[b] and cnt == min(max(pl.n_out[b] - st.y_lo, 0), st.y_hi - st.y_lo)
            y_done[b] += cnt
            done_count[b] += int(done)
            assert (y_done[b] == pl.n_out[b]) == (done_count[b] == 1), "done with the row's last sample, once"
        prev = st
    last = pl.steps[-1]
    assert last.m_hi == last.p_hi == last.y_hi == max(pl.n_out), "the last step flushes all three"
    assert y_done == pl.n_out and done_count == [1] * B
    assert pl.max_chunk == max(st.y_hi - st.y_lo for st in pl.steps)
    if len(pl.steps) > 2 and W == 1:  # the delay is the reach and the window, no more
        mid = pl.steps[len(pl.steps) // 2]
        if mid.m_hi > EREACH and any(d < n for d, n in zip(mid.den_final, lens)):
            assert mid.p_hi == mid.m_hi - EREACH and mid.y_hi == mid.p_hi


def test_plan_without_limiter_is_unchanged_and_refusals():
    lens = [61, 32, 17, 1, 0, 45]
    a = sp.plan(lens, 16, 8, 320, 441, _half(320, 441), reach=13)
    b = sp.plan(lens, 16, 8, 320, 441, _half(320, 441), reach=13, env_reach=None, window=None)
    assert a == b and a.env_reach is None and a.window is None
    assert all(st.p_hi is None and st.y_hi is None for st in a.steps)
    # new fields have defaults: a Step built as before this change still is one
    st = sp.Step(0, 0, 4, sp.Windows(), None, 0, 10, [4], [4], [10])
    assert st.delivered == (0, 10) and st.out_counts([7]) == [(0, 7, True)]
    for kw in (dict(env_reach=10), dict(window=80), dict(env_reach=-1, window=80), dict(env_reach=10, window=0)):
        with pytest.raises(ValueError):
            sp.plan(lens, 16, reach=13, **kw)


# ---- the two range stages in numpy, along a plan ------------------------------------------------------------------

def _simulate(rows, pl, g, W, ereach_used=None, window_used=None):
    """The stitched buffers start as poison. Step c: the resampled buffer receives r[:M_c]; the envelope of
    [p_lo, p_hi) is computed from that buffer, the gain curve and the product of [y_lo, y_hi) from the envelope
    buffer; both clipped to the row. ereach_used / window_used shift the ranges as a plan with a reach / window
    shorter by one would. -> the concatenated chunks of every row"""
    de = 0 if ereach_used is None else EREACH - ereach_used
    dw = 0 if window_used is None else W - window_used
    out = []
    for b, r in enumerate(rows):
        n = len(r)
        assert n == pl.n_out[b]
        res = np.full(n, POISON, np.float32)
        env = np.full(n, POISON, np.float32)
        got = []
        p_lo = y_lo = 0
        for st in pl.steps:
            last = st is pl.steps[-1]
            m = min(st.m_hi, n)
            res[:m] = r[:m]
            p_hi = min(st.p_hi + (de if st.p_hi and not last else 0), n)
            y_hi = min(st.y_hi + (de + dw if st.y_hi and not last else 0), n)
            p_lo, y_lo = min(p_lo, p_hi), min(y_lo, y_hi)
            if p_hi > p_lo:
                env[p_lo:p_hi] = lm.envelope_ref(res)[p_lo:p_hi]
            if y_hi > y_lo:
                s = lm.gain_curve_ref(env, g, C32, W)[y_lo:y_hi]
                got.append(lm.apply_ref(res[y_lo:y_hi], g, s))
            p_lo, y_lo = p_hi, y_hi
        out.append(np.concatenate(got) if got else np.zeros(0, np.float32))
    return out


@pytest.mark.parametrize("rate,W,chunk,first", [(8000, 80, 2, 1), (16000, 80, 3, None), (22050, 1, 2, None),
                                                 (48000, 2, 1, None), (8000, 2048, 2, None)])
def test_range_stages_along_a_plan_are_the_one_pass_result(rate, W, chunk, first):
    up, down = RATES[rate]
    half = _half(up, down)
    lens = [9, 4, 0, 1]
    pl = sp.plan(lens, chunk, first, up, down, half, reach=1, denoise=False, env_reach=EREACH, window=W)
    assert len(pl.steps) > 2
    rows = [_row(n, 20 + b) for b, n in enumerate(pl.n_out)]
    db = 12.0
    g = lm.fixed_gain_ref(db)
    want = [lm.limit_fixed_ref(r, db, C_DB, W)[0] for r in rows]
    assert lm.limit_fixed_ref(rows[0], db, C_DB, W)[1] < 1.0
    got = _simulate(rows, pl, g, W)
    for b in range(len(lens)):
        assert got[b].shape == want[b].shape and np.array_equal(got[b], want[b]), b
    # negative controls: ranges that run one sample further than the reach / the window allow read the poison
    assert not np.array_equal(_simulate(rows, pl, g, W, ereach_used=EREACH - 1)[0], want[0])
    if W < pl.n_out[0]:
        assert not np.array_equal(_simulate(rows, pl, g, W, window_used=W - 1)[0], want[0])


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_audio_output_fixed_gain_arguments():
    from hifigan.output import AudioOut, AudioOutput, Limited
    o = AudioOutput(16000, gain_db=6.0)
    assert o.gain_db == 6.0 and o.limiter is None and o.normalize is None and o.loudness is None
    o = AudioOutput(16000, gain_db=6, true_peak=-1.0, limiter=5.0, limiter_passes=7)
    assert o.gain_db == 6.0 and o.limiter_window == 80
    assert AudioOutput(8000, gain_db=-3.0, limiter=256.0).limiter_window == 2048
    assert AudioOutput(16000).gain_db is None
    for kw in (dict(gain_db=6.0, normalize="peak"), dict(gain_db=6.0, normalize="rms"),
               dict(gain_db=6.0, loudness=-16.0), dict(gain_db=float("nan")), dict(gain_db=float("inf")),
               dict(gain_db=6.0, limiter=0.0), dict(gain_db=6.0, limiter=128.1),
               dict(limiter=5.0), dict(limiter=5.0, normalize="rms")):
        with pytest.raises(ValueError):
            AudioOutput(16000, **kw)
    assert AudioOut._fields == ("audio", "lengths", "sample_rate", "gain")
    assert Limited._fields == ("audio", "lengths", "sample_rate", "gain", "reduction", "trim")
    # the per-row override: converted on the host by fixed_gain_ref
    g = o.fixed_gain(3, "cpu", [0.0, 6.0, -20.0])
    assert g.dtype == torch.float32 and g.tolist() == [float(lm.fixed_gain_ref(v)) for v in (0.0, 6.0, -20.0)]
    assert o.fixed_gain(2, "cpu").tolist() == [float(lm.fixed_gain_ref(6.0))] * 2
    assert o.fixed_gain(2, "cpu", torch.tensor([1.0, 2.0])).tolist() == \
        [float(lm.fixed_gain_ref(1.0)), float(lm.fixed_gain_ref(2.0))]
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, float("nan")], [float("inf"), 0.0]):
        with pytest.raises(ValueError):
            o.fixed_gain(2, "cpu", bad)
    x = torch.zeros(2, 512)
    lens = torch.tensor([512, 100], dtype=torch.int32)
    plain = AudioOutput(16000, loudness=-16, limiter=5.0)
    for fn in (lambda: AudioOutput(16000)(x, None, gain_db=[1.0, 2.0]),
               lambda: AudioOutput(16000).finish(x, lens, gain_db=[1.0, 2.0]),
               lambda: plain(x, None, gain_db=[1.0, 2.0]),
               lambda: plain.limited(x, lens, gain_db=[1.0, 2.0])):
        with pytest.raises(ValueError, match="without gain_db"):
            fn()
    with pytest.raises(ValueError, match="without limiter"):
        AudioOutput(16000, gain_db=6.0).limited(x, lens)


def test_runtime_range_wrappers_refuse_host_tensors():
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    x = torch.zeros(2, 512)
    for fn in (lambda: rt.peak_envelope_range(x, None, None, 0, 4, x.clone()),
               lambda: rt.limit_range(x, x.clone(), None, torch.ones(2), 0.89, 80, 0, 4, torch.ones(2)),
               lambda: AudioOutput(16000, gain_db=6.0, limiter=5.0)(x)):
        with pytest.raises(HipPathError):
            fn()


def test_wave_streamer_arguments():
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    g = make_generator("bf16")
    for o, what in ((AudioOutput(16000, normalize="peak"), "whole utterance"),
                    (AudioOutput(16000, loudness=-16.0), "whole utterance"),
                    (AudioOutput(16000, loudness=-16.0, limiter=5.0), "whole utterance")):
        with pytest.raises(ValueError, match=what):
            WaveStreamer(g, None, o)
    s = WaveStreamer(g, None, AudioOutput(16000, gain_db=6.0, limiter=5.0), chunk_frames=16)
    assert s.fixed_gain and s.limited and s.reduction is None
    s1 = WaveStreamer(g, None, AudioOutput(16000, gain_db=6.0), chunk_frames=16)
    assert s1.fixed_gain and not s1.limited
    s0 = WaveStreamer(g, None, AudioOutput(16000), chunk_frames=16)
    assert not s0.fixed_gain and not s0.limited
    mel = torch.zeros(2, 80, 8)
    for st in (s0, WaveStreamer(g, chunk_frames=16)):
        with pytest.raises(ValueError, match="without gain_db"):
            st(mel, [8, 4], gain_db=[0.0, 1.0])


def test_c_abi_refuses_bad_range_arguments_before_any_launch():
    from matcha_hip import runtime as rt
    L = rt.lib()
    assert L.mt_abi_version() == 1  # a pure addition
    p, p2, p3, p4 = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4))  # never dereferenced

    def last():
        return L.mt_last_error().decode()

    def env(B=1, Ln=4000, half=40, i_lo=0, cnt=100, audio=p, taps=p, out=p2, ws=p3, ws_bytes=1 << 20):
        return L.mt_peak_envelope_range(audio, B, Ln, None, taps, half, i_lo, cnt, out, ws, ws_bytes, None)

    assert env(B=0) != 0 and "peak_envelope_range: B 0" in last()
    assert env(B=65536) != 0 and "peak_envelope_range: B 65536" in last()
    assert env(Ln=0) != 0 and "L 0" in last()
    assert env(Ln=1 << 29) != 0 and "peak_envelope_range: B" in last()
    assert env(half=0) != 0 and "half-length 0" in last()
    assert env(half=1025) != 0 and "half-length 1025" in last()
    assert env(i_lo=-1) != 0 and "peak_envelope_range: samples [-1" in last()
    assert env(cnt=0) != 0 and "peak_envelope_range: samples" in last()
    assert env(cnt=-5) != 0 and "peak_envelope_range: samples" in last()
    assert env(i_lo=(1 << 31) - 100, cnt=100) != 0 and "peak_envelope_range: samples" in last()
    assert env(i_lo=(1 << 30), cnt=(1 << 30)) != 0 and "peak_envelope_range: samples" in last()
    for kw in (dict(audio=None), dict(taps=None), dict(out=None)):
        assert env(**kw) != 0 and "null argument" in last(), kw
    assert env(out=p) != 0 and "overlaps" in last()
    assert env(out=ctypes.c_void_p((1 << 24) + 4 * 3999)) != 0 and "overlaps" in last()
    assert env(ws=None) != 0 and "workspace" in last()
    assert env(ws=ctypes.c_void_p((3 << 24) + 8)) != 0 and "16-byte aligned" in last()
    assert env(ws_bytes=L.mt_peak_envelope_workspace_bytes() - 1) != 0 and "workspace too small" in last()

    def lim(B=1, Ln=4000, W=80, ceiling=0.89, i_lo=0, cnt=100, audio=p, e=p2, gain=p, out=p3, out_cnt=p, red=p,
            ws=p4, ws_bytes=1 << 20):
        return L.mt_limit_range(audio, e, B, Ln, None, gain, ceiling, W, i_lo, cnt, out, out_cnt, red, ws, ws_bytes,
                                None)

    assert lim(B=0) != 0 and "limit_range: B 0" in last()
    assert lim(B=65536) != 0 and "limit_range: B 65536" in last()
    assert lim(Ln=0) != 0 and "L 0" in last()
    assert lim(Ln=1 << 29) != 0 and "limit_range: B" in last()
    for W in (0, -1, 2049):
        assert lim(W=W) != 0 and f"window of {W} samples" in last()
    assert lim(i_lo=-1) != 0 and "limit_range: samples [-1" in last()
    assert lim(cnt=0) != 0 and "limit_range: samples" in last()
    assert lim(i_lo=(1 << 31) - 100, cnt=100) != 0 and "limit_range: samples" in last()
    for v in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        assert lim(ceiling=v) != 0 and "ceiling" in last(), v
    for kw in (dict(audio=None), dict(e=None), dict(gain=None), dict(out=None), dict(out_cnt=None), dict(red=None)):
        assert lim(**kw) != 0 and "null argument" in last(), kw
    assert lim(out=p) != 0 and "overlaps" in last()
    assert lim(out=p2) != 0 and "overlaps" in last()
    assert lim(out=ctypes.c_void_p((1 << 24) - 16)) != 0 and "overlaps" in last()       # out's end inside audio
    assert lim(out=ctypes.c_void_p((2 << 24) + 4 * 3999)) != 0 and "overlaps" in last()  # out's start inside env
    assert lim(ws=None) != 0 and "workspace" in last()
    assert lim(ws=ctypes.c_void_p((4 << 24) + 4)) != 0 and "16-byte aligned" in last()
    need = L.mt_limit_range_workspace_bytes(3, 2 * rt.LIMIT_TILE + 1, 80)
    assert need == 3 * 3 * 4  # one minimum per tile of the range
    assert lim(B=3, cnt=2 * rt.LIMIT_TILE + 1, ws_bytes=need - 1) != 0 and "workspace too small" in last()
    assert L.mt_limit_range_workspace_bytes(1, 100, 80) == 4
    assert L.mt_limit_range_workspace_bytes(0, 100, 80) == 0 and "B 0" in last()
    assert L.mt_limit_range_workspace_bytes(1, 0, 80) == 0 and "cnt 0" in last()
    assert L.mt_limit_range_workspace_bytes(1, 100, 2049) == 0 and "window of 2049" in last()
