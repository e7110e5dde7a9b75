"""Look-ahead true-peak limiter, host side (CPU only: no kernel launches): the specification in matcha_hip/limiter.py
 against its own stated properties, and the argument checks of the C ABI and of AudioOutput."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

from matcha_hip import audio_out as ao
from matcha_hip import limiter as lm
from matcha_hip import loudness as ld

WINDOWS = (1, 2, 7, 80, 2048)
ONE = lm.ONE
C32 = np.float32(10.0 ** (-1.0 / 20.0))


def burst_signal(fs=16000, seed=0):
    """2 s of noise of sigma 0.02 with twelve 8-sample bursts of sigma 0.5: speech-shaped in the one respect that
    matters here, more than 15 dB between its loudness and its peaks"""
    rng = np.random.default_rng(seed)
    n = 2 * fs
    x = rng.standard_normal(n) * 0.02
    for p in rng.choice(np.arange(200, n - 200, 400), 12, replace=False):
        x[p:p + 8] = rng.standard_normal(8) * 0.5
    return x.astype(np.float32)


def _envelope_by_definition(x):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(ld.oversample4_ref(x))
    n = len(x)
    p = np.zeros(n, dtype=np.float32)
    for i in range(n):
        v = [abs(x[i])] + [r[m] for m in range(4 * i - 3, 4 * i + 4) if 0 <= m < 4 * n]
        v = [t for t in v if not np.isnan(t)]
        p[i] = max(v) if v else 0.0
    return p


def test_envelope_is_the_true_peak_meter_seen_per_sample():
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 257):
        x = (rng.standard_normal(n) * 0.3).astype(np.float32)
        p = lm.envelope_ref(x)
        assert p.dtype == np.float32 and p.shape == (n,)
        assert np.array_equal(p, _envelope_by_definition(x))
        assert p.max() == ld.true_peak_ref(x)  # every 4x output lies in some sample's reach
        assert (p >= np.abs(x)).all()
    assert lm.envelope_ref(np.zeros(0)).shape == (0,)
    # a NaN counts as absent, an infinity does not
    x = (rng.standard_normal(200) * 0.3).astype(np.float32)
    x[50], x[120] = np.nan, np.inf
    p = lm.envelope_ref(x)
    assert not np.isnan(p).any() and p[50] == 0.0 and p[120] == np.inf
    assert np.array_equal(p, _envelope_by_definition(x))
    assert np.array_equal(p[180:], lm.envelope_ref(np.concatenate([np.zeros(150, np.float32), x[150:]]))[180:])


def test_window_samples():
    assert lm.window_samples(16000, 5.0) == 80 and lm.window_samples(22050, 5.0) == 110
    assert lm.window_samples(8000, 0.01) == 1 and lm.window_samples(8000, 256.0) == 2048
    assert lm.window_samples(22050, 0.0681) == 2  # rint(1.5016)
    for fs, ms in ((8000, 256.1), (48000, 50.0), (16000, 0.0), (16000, -1.0), (16000, float("nan")),
                   (16000, float("inf"))):
        with pytest.raises(ValueError):
            lm.window_samples(fs, ms)
    for W in (0, 2049, -3):
        with pytest.raises(ValueError):
            lm.gain_curve_ref(np.ones(4, np.float32), 1.0, C32, W)


@pytest.mark.parametrize("W", WINDOWS)
def test_reduction_never_exceeds_the_quotient(W):
    rng = np.random.default_rng(W)
    for n, scale, g0 in ((3000, 0.3, 4.0), (5000, 0.05, 30.0), (700, 1.0, 1.0)):
        p = np.abs(rng.standard_normal(n) * scale).astype(np.float32)
        r = lm.quotient_ref(p, g0, C32)
        s = lm.gain_curve_ref(p, g0, C32, W)
        assert s.dtype == np.float32 and s.shape == (n,)
        assert (r < 1).any() and (s <= r).all() and (s > 0).all() and (s <= 1).all()
        a = np.float32(g0) * p
        assert (a * s <= C32 * np.float32(1 + 2.0 ** -22)).all()  # the limited envelope, up to the product's rounding
        if W == 1:
            assert np.array_equal(s, (np.floor(r.astype(np.float64) * ONE) / ONE).astype(np.float32))


def test_nothing_over_the_ceiling_leaves_the_gain_alone():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4000) * 0.05).astype(np.float32)
    p = lm.envelope_ref(x)
    g0 = np.float32(0.85 / p.max())
    assert (g0 * p).max() < C32
    for W in WINDOWS:
        s = lm.gain_curve_ref(p, g0, C32, W)
        assert (s == 1.0).all()
        assert np.array_equal(lm.apply_ref(x, g0, s), g0 * x)
    # ... and a reduction reaches no further than W - 1 samples
    p2 = p.copy()
    p2[2000] = np.float32(3.0) / g0
    for W in (1, 7, 80):
        s = lm.gain_curve_ref(p2, g0, C32, W)
        assert (s[:2000 - W + 1] == 1.0).all() and (s[2000 + W:] == 1.0).all()
        assert (s[2000 - W + 1:2000 + W] < 1.0).all()


@pytest.mark.parametrize("W", (1, 2, 7, 80, 2048))
@pytest.mark.parametrize("where", ("middle", "first", "last"))
def test_one_peak_gives_linear_ramps(W, where):
    n = 5000
    k = {"middle": 2500, "first": 0, "last": n - 1}[where]
    p = np.full(n, 0.01, dtype=np.float32)
    p[k] = 2.5
    g0 = np.float32(1.7)
    a = g0 * p[k]
    qk = int(math.floor(float(C32 / a) * ONE))
    s = lm.gain_curve_ref(p, g0, C32, W)
    d = np.abs(np.arange(n) - k)
    S = np.where(d < W, W * ONE - (W - d) * (ONE - qk), W * ONE)  # W - d windows of the sum hold the peak
    assert np.array_equal(s, (S.astype(np.float64) / float(W * ONE)).astype(np.float32))
    assert s[k] == np.float32(qk / ONE) and s[k] <= C32 / a
    assert (s[d >= W] == 1.0).all()
    if W > 2 and where == "middle":
        assert (np.diff(s[k:k + W]) > 0).all() and (np.diff(s[k - W + 1:k + 1]) < 0).all()


def test_short_rows():
    assert lm.gain_curve_ref(np.zeros(0, np.float32), 2.0, C32, 80).shape == (0,)
    assert lm.apply_ref(np.zeros(0, np.float32), 2.0, np.zeros(0, np.float32)).shape == (0,)
    for W in WINDOWS:
        assert lm.gain_curve_ref(np.float32([0.1]), 2.0, C32, W)[0] == 1.0
        s = lm.gain_curve_ref(np.float32([3.0]), 2.0, C32, W)
        q = int(math.floor(float(C32 / np.float32(6.0)) * ONE))
        assert s[0] == np.float32(q / ONE)  # every window of the sum holds the one sample
    # W > n: every window holds the peak wherever both lie inside the row
    p = np.float32([0.1, 0.1, 3.0, 0.1, 0.1])
    s = lm.gain_curve_ref(p, 2.0, C32, 2048)
    d = np.abs(np.arange(5) - 2)
    want = ((2048 * ONE - (2048 - d) * (ONE - q)) / float(2048 * ONE)).astype(np.float32)
    assert np.array_equal(s, want)
    y, g, red, trim = lm.limiter_ref(np.zeros(0, np.float32), 16000, -16.0, -1.0, 80)
    assert y.shape == (0,) and g == 1.0 and red == 1.0 and trim == 1.0
    for row in (np.zeros(4000, np.float32), np.full(4000, 1e-5, np.float32)):
        y, g, red, trim = lm.limiter_ref(row, 8000, -16.0, -1.0, 40)  # silent or fully gated: untouched
        assert np.array_equal(y, row) and g == 1.0 and red == 1.0 and trim == 1.0


def test_nan_and_inf():
    p = np.float32([0.1, np.inf, 0.1, 0.1, 3.0, 0.1])
    r = lm.quotient_ref(p, 2.0, C32)
    assert r[1] == 0.0 and r[0] == 1.0 and r[4] == C32 / np.float32(6.0)
    s = lm.gain_curve_ref(p, 2.0, C32, 2)
    assert s[1] == 0.0 and s[0] == 0.5 and s[2] == 0.5 and (s <= r).all()
    # a NaN product is not over the ceiling
    assert (lm.quotient_ref(np.float32([np.inf, 1.0]), 0.0, C32) == 1.0).all()
    assert (lm.quotient_ref(np.float32([np.nan, 0.1]), 2.0, C32) == 1.0).all()
    x = np.float32([0.5, np.nan, -np.inf, 0.25])
    y = lm.apply_ref(x, 2.0, np.float32([1.0, 0.5, 0.5, 0.0]))
    assert y[0] == 1.0 and np.isnan(y[1]) and y[2] == -np.inf and y[3] == 0.0


def test_apply_rounds_two_products():
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(20000) * 0.2).astype(np.float32)
    s = rng.uniform(0.1, 1.0, 20000).astype(np.float32)
    g0 = np.float32(3.1415927)
    y = lm.apply_ref(x, g0, s)
    t = (g0 * x).astype(np.float32)
    assert np.array_equal(y, t * s)
    # one product rounded once (the fp64 product of g0 and x is exact) differs on a good share of the samples
    fused = (x.astype(np.float64) * float(g0) * s.astype(np.float64)).astype(np.float32)
    differ = int((fused != y).sum())
    print(f"{differ} of {x.size} samples would differ with a single rounding")
    assert differ > 1000
    assert np.abs(fused.astype(np.float64) - y).max() <= np.abs(y).max() * 2.0 ** -23


_BURST = {}


def _burst_run(fs=16000):
    if fs not in _BURST:
        x = burst_signal(fs)
        W = lm.window_samples(fs, 5.0)
        trace = []
        y, g, red, trim = lm.limiter_ref(x, fs, -16.0, -1.0, W, 3, trace=trace)
        _BURST[fs] = (x, W, y, g, red, trim, trace)
    return _BURST[fs]


def test_make_up_passes_close_in_on_the_target():
    x, W, y, g, red, trim, trace = _burst_run()
    assert W == 80 and len(trace) == 3
    E, _ = ld.loudness_ref(x, 16000)
    TP = ld.true_peak_ref(x)
    capped = ld.lufs(ld.loudness_ref(ao.f32_ref(x, ld.loudness_gain_ref(E, TP, -16.0, -1.0)), 16000)[0])
    got = [ld.lufs(Ek) for _, Ek in trace]
    err = [abs(v + 16.0) for v in got]
    print(f"capped gain: {capped:.3f} LUFS; passes: {', '.join(f'{v:.3f}' for v in got)}; g {g:.4f}, "
          f"reduction {red:.4f}, trim {trim:.6f}")
    assert err[0] > err[1] > err[2]
    assert err[2] < abs(capped + 16.0)
    assert trace[0][0] == ld.loudness_gain_ref(E, TP, -16.0, -1.0, limit=False)
    assert trace[1][0] == lm.next_gain_ref(trace[0][0], ld.target_level(-16.0), trace[0][1])
    assert trace[2][0] == g and 0 < red < 1 and 0 < trim <= 1
    # the same call with fewer passes stops earlier on the same path
    y1, g1, _, _ = lm.limiter_ref(x, 16000, -16.0, -1.0, W, 1)
    assert g1 == trace[0][0] and ld.lufs(ld.loudness_ref(y1, 16000)[0]) == got[0]
    p = lm.envelope_ref(x)
    s = lm.gain_curve_ref(p, g, C32, W)
    assert (s <= lm.quotient_ref(p, g, C32)).all() and s.min() == red
    for bad in (0, 9):
        with pytest.raises(ValueError):
            lm.limiter_ref(x[:100], 16000, -16.0, -1.0, W, bad)


def test_trimmed_true_peak_is_at_or_under_the_ceiling():
    """TP' trim <= c, the product taken exactly (two fp32 factors in fp64) against c = 10^(-1/20). The trim is
    float32(1 / float32(TP' (1 + eps) / c)) with eps = trim_headroom of the 4x filter, so the product is at most
    c (1 - eps + 2^-23); and what the meter reads on the delivered signal clamp(trim y) is at or under c as well."""
    x, W, y, g, red, trim, trace = _burst_run()
    c = 10.0 ** (-1.0 / 20.0)
    eps = lm.default_headroom()
    u = 2.0 ** -24
    h, half = ao.design_filter(4, 1)
    P = ao.polyphase(h.astype(np.float32), half, 4)
    A = np.abs(P.astype(np.float64)).sum(axis=1).max()
    assert P.shape == (4, 21) and eps == lm.trim_headroom(P) == (2 * 23 * A + 4) * u and 4e-6 < eps < 1e-5
    TPp = ld.true_peak_ref(y)
    delivered = ld.true_peak_ref(ao.f32_ref(y, trim))
    print(f"TP' / c = {float(TPp) / c:.7f}, trim = {float(trim):.8f}, eps = {eps:.2e}, TP' trim / c - 1 = "
          f"{float(TPp) * float(trim) / c - 1.0:+.2e}, delivered TP / c - 1 = {float(delivered) / c - 1.0:+.2e}")
    assert trim == lm.trim_ref(TPp, 1.0, -1.0, eps) and trim < 1.0  # the smoothing lets a fraction of a percent through
    assert lm.trim_ref(TPp, 0.0, -1.0, eps) == 1.0 and lm.trim_ref(np.float32(0.5), 1.0, -1.0, eps) == 1.0
    assert float(TPp) / c < 1.01
    assert float(TPp) * float(trim) <= c
    assert float(TPp) * float(trim) >= c * (1.0 - eps - 2 * u)  # and no further under it than the headroom
    assert float(delivered) <= c


def test_tile_constants_mirror_the_kernels():
    from matcha_hip import runtime as rt
    src = open(os.path.join(REPO, "matcha-tts_amd", "csrc", "mt_limiter.hip")).read()
    for name, want in (("LM_ENV_T", rt.ENVELOPE_TILE), ("LM_T", rt.LIMIT_TILE), ("LM_MAX_W", rt.LIMIT_MAX_WINDOW)):
        m = re.search(rf"constexpr int {name} = (\d+);", src)
        assert m and int(m.group(1)) == want, name
    assert rt.LIMIT_MAX_WINDOW == lm.MAX_WINDOW
    m = re.search(r"constexpr int LM_MAX_L = \(1 << 29\) - (\d+);", src)
    tp = re.search(r"constexpr int TP_MAX_L = \(1 << 29\) - TP_TN;",
                   open(os.path.join(REPO, "matcha-tts_amd", "csrc", "mt_loudness.hip")).read())
    assert m and tp and int(m.group(1)) == rt.RESAMPLE_TILE  # the true-peak kernel's range
    assert "#pragma clang fp contract(off)" in src
    mk = open(os.path.join(REPO, "matcha-tts_amd", "Makefile")).read()
    assert "csrc/mt_limiter.hip" in mk and "fast-math" not in mk and "-ffp-contract" not in mk


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from matcha_hip import runtime as rt
    L = rt.lib()
    assert L.mt_abi_version() == 1
    p, p2, p3 = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)  # never dereferenced

    def last():
        return L.mt_last_error().decode()

    def env(B=1, Ln=4000, half=40, audio=p, taps=p, out=p2, ws=p3, ws_bytes=1 << 20):
        return L.mt_peak_envelope(audio, B, Ln, None, taps, half, out, ws, ws_bytes, None)

    assert env(B=0) != 0 and "peak_envelope: B 0" in last()
    assert env(B=65536) != 0 and "peak_envelope: B 65536" in last()
    assert env(Ln=0) != 0 and "L 0" in last()
    assert env(Ln=1 << 29) != 0 and "peak_envelope: B" in last()
    assert env(half=0) != 0 and "half-length 0" in last()
    assert env(half=1025) != 0 and "half-length 1025" in last()
    for kw in (dict(audio=None), dict(taps=None), dict(out=None)):
        assert env(**kw) != 0 and "null argument" in last(), kw
    assert env(out=p) != 0 and "overlaps" in last()
    assert env(out=ctypes.c_void_p((1 << 20) + 4 * 3999)) != 0 and "overlaps" in last()
    assert env(ws=None) != 0 and "workspace" in last()
    assert env(ws=ctypes.c_void_p((3 << 20) + 8)) != 0 and "16-byte aligned" in last()
    need = L.mt_peak_envelope_workspace_bytes()
    assert need == 4 * (4 * 513)  # the table of the longest filter
    assert env(ws_bytes=need - 1) != 0 and "workspace too small" in last()

    def lim(B=1, Ln=4000, W=80, level=0.1, ceiling=0.89, audio=p, e=p2, peak=p, meansq=p, gain_in=None, out=p3,
            red=p, gain=p, ws=p, ws_bytes=1 << 20):
        return L.mt_limit(audio, e, B, Ln, None, peak, meansq, gain_in, level, ceiling, W, out, red, gain, ws,
                          ws_bytes, None)

    assert lim(B=0) != 0 and "limit: B 0" in last()
    assert lim(B=65536) != 0 and "limit: B 65536" in last()
    assert lim(Ln=0) != 0 and "L 0" in last()
    assert lim(Ln=1 << 29) != 0 and "limit: B" in last()
    for W in (0, -1, 2049):
        assert lim(W=W) != 0 and f"window of {W} samples" in last()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert lim(level=v) != 0 and "level" in last(), v
        assert lim(ceiling=v) != 0 and "ceiling" in last(), v
    assert lim(ceiling=1e-60) != 0 and "ceiling" in last()  # not a positive fp32 value
    for kw in (dict(audio=None), dict(e=None), dict(peak=None), dict(meansq=None), dict(out=None), dict(red=None),
               dict(gain=None)):
        assert lim(**kw) != 0 and "null argument" in last(), kw
    assert lim(out=p) != 0 and "overlaps" in last()
    assert lim(out=p2) != 0 and "overlaps" in last()
    assert lim(out=ctypes.c_void_p((1 << 20) - 16)) != 0 and "overlaps" in last()
    assert lim(ws=None) != 0 and "workspace" in last()
    assert lim(ws=ctypes.c_void_p((1 << 20) + 4)) != 0 and "16-byte aligned" in last()
    need = L.mt_limit_workspace_bytes(3, 2 * rt.LIMIT_TILE + 1, 80)
    assert need == 3 * 3 * 4  # one minimum per tile
    assert lim(B=3, Ln=2 * rt.LIMIT_TILE + 1, ws_bytes=need - 1) != 0 and "workspace too small" in last()
    assert L.mt_limit_workspace_bytes(0, 100, 80) == 0 and "B 0" in last()
    assert L.mt_limit_workspace_bytes(1, 100, 2049) == 0 and "window of 2049" in last()
    assert L.mt_limit_workspace_bytes(1, 1 << 29, 80) == 0 and "limit: B" in last()


def test_audio_output_argument_refusals():
    from hifigan.output import AudioOut, AudioOutput, Limited
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    o = AudioOutput(16000, loudness=-16, limiter=5.0)
    assert o.limiter == 5.0 and o.limiter_window == 80 and o.limiter_passes == 3
    d = AudioOutput(16000, loudness=-16)
    assert d.limiter is None and d.limiter_window is None and d.limiter_passes == 3
    assert AudioOutput(22050, loudness=-16, limiter=5, limiter_passes=8).limiter_window == 110
    assert AudioOutput(8000, source_rate=8000, loudness=-16, limiter=256.0).limiter_window == 2048
    for kw in (dict(limiter=5.0), dict(limiter=5.0, normalize="rms"), dict(loudness=-16, limiter=0.0),
               dict(loudness=-16, limiter=-5.0), dict(loudness=-16, limiter=float("nan")),
               dict(loudness=-16, limiter=float("inf")), dict(loudness=-16, limiter=128.1),
               dict(loudness=-16, limiter=5.0, limiter_passes=0), dict(loudness=-16, limiter=5.0, limiter_passes=9),
               dict(loudness=-16, limiter=5.0, limiter_passes=2.5), dict(limiter_passes=0)):
        with pytest.raises(ValueError):
            AudioOutput(16000, **kw)
    assert AudioOut._fields == ("audio", "lengths", "sample_rate", "gain")
    assert Limited._fields == ("audio", "lengths", "sample_rate", "gain", "reduction", "trim")
    x = torch.zeros(2, 512)
    lens = torch.tensor([512, 100], dtype=torch.int32)
    with pytest.raises(ValueError, match="without limiter"):
        d.limited(x, lens)
    for fn in (lambda: o(x), lambda: o.finish(x, lens), lambda: o.limited(x, lens),
               lambda: rt.peak_envelope(x, None, None),
               lambda: rt.limit(x, x, None, (x[:, 0], x[:, 0].double()), 0.1, 0.89, 80)):
        with pytest.raises(HipPathError):
            fn()
