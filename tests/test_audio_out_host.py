"""Audio output stage, host side (CPU only: no kernel launches): the specification in matcha_hip/audio_out.py
 against scipy's polyphase resampler and against its own defining formulas, the G.711 / PCM16
encodings exhaustively, and the argument checks of the C ABI and of AudioOutput."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

from matcha_hip import audio_out as ao

RATES = (8000, 11025, 16000, 24000, 32000, 44100, 48000)
SRC = 22050


def test_rates_and_refusals():
    assert [ao.rates(SRC, d) for d in RATES] == [(160, 441), (1, 2), (320, 441), (160, 147), (640, 441), (2, 1),
                                                 (320, 147)]
    assert ao.rates(SRC, SRC) == (1, 1)
    for src, dst in ((22050, 22051), (22050, 1025 * 22050), (44100, 1)):
        with pytest.raises(ValueError):
            ao.rates(src, dst)
    assert ao.out_length(0, 320, 441) == 0 and ao.out_length(1, 320, 441) == 1 and ao.out_length(441, 320, 441) == 320
    assert ao.out_length(442, 320, 441) == 321


def test_filter_and_resampler_pin_against_scipy():
    """design_filter is the filter scipy.signal.resample_poly designs by default, and resample_ref is resample_poly
    with that filter given (scipy multiplies a given window by `up` itself), at the seven rates."""
    pytest.importorskip("scipy")
    from scipy import signal
    rng = np.random.default_rng(5)
    for dst in RATES:
        up, down = ao.rates(SRC, dst)
        h, half = ao.design_filter(up, down)
        assert half == 10 * max(up, down) and h.shape == (2 * half + 1,) and h.dtype == np.float64
        want = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        e_h = np.abs(h - want).max()
        assert abs(h.sum() - up) < 1e-12 * up
        worst = 0.0
        for n in (1, 7, 300, 1025):
            x = rng.uniform(-1, 1, n)
            y = ao.resample_ref(x, up, down, h, half)
            ref = signal.resample_poly(x, up, down, window=h / up)
            assert y.shape == ref.shape == (ao.out_length(n, up, down),)
            worst = max(worst, np.abs(y - ref).max())
        print(f"{SRC}->{dst}: filter {e_h:.1e}, resample {worst:.1e}")
        assert e_h <= 1e-12 and worst <= 1e-12, (dst, e_h, worst)


@pytest.mark.parametrize("dst", RATES)
def test_unit_impulse_returns_the_taps(dst):
    up, down = ao.rates(SRC, dst)
    h, half = ao.design_filter(up, down)
    n = 37
    for k0 in (0, 1, n - 1):
        x = np.zeros(n)
        x[k0] = 1.0
        y = ao.resample_ref(x, up, down, h, half)
        j = half + np.arange(y.shape[0]) * down - k0 * up
        ok = (j >= 0) & (j <= 2 * half)
        want = np.where(ok, h[np.clip(j, 0, 2 * half)], 0.0)
        assert np.array_equal(y, want), (dst, k0)
        assert ok.any()


def test_polyphase_table():
    h = np.arange(1, 12, dtype=np.float64)  # half = 5, 11 taps
    P = ao.polyphase(h, 5, 4)
    assert P.shape == (4, 3)
    assert P.tolist() == [[1, 5, 9], [2, 6, 10], [3, 7, 11], [4, 8, 0]]
    assert ao.polyphase(h, 5, 1).tolist() == [h.tolist()]


def test_mulaw_exhaustive():
    q = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    u = ao.mulaw_ref(q)
    assert u.dtype == np.uint8 and u.shape == q.shape
    # known codes (ITU-T G.711 / the classic linear2ulaw): silence, the extremes, the first segment boundaries
    known = {0: 0xFF, -1: 0x7F, 32767: 0x80, -32768: 0x00, 32635: 0x80, -32635: 0x00, 3: 0xFF, 4: 0xFE, 123: 0xF0,
             124: 0xEF, -4: 0x7E, 1000: 0xCE}
    for s, byte in known.items():
        assert int(ao.mulaw_ref(np.int16(s))) == byte, (s, hex(int(ao.mulaw_ref(np.int16(s)))))
    # the decode table: every byte decodes to a sample that encodes back to the same byte (0x7F, "negative zero",
    # decodes to 0, whose code is 0xFF)
    table = ao.mulaw_decode(np.arange(256, dtype=np.uint8))
    back = ao.mulaw_ref(table)
    for b in range(256):
        assert int(back[b]) == (0xFF if b == 0x7F else b), b
    # every sample decodes to within half its segment's step of itself (below the clip)
    dec = table[u].astype(np.int32)
    seg = ((~u >> 4) & 7).astype(np.int32)
    inside = np.abs(q.astype(np.int32)) <= ao.MULAW_CLIP
    assert (np.abs(dec - q)[inside] <= (4 << seg[inside])).all()
    # monotone within each sign: the magnitude code (the inverted low seven bits) never decreases with |sample|
    code = (~u) & 0x7F
    pos, neg = q >= 0, q < 0
    assert (np.diff(code[pos].astype(np.int32)) >= 0).all()
    assert (np.diff(code[neg].astype(np.int32)) <= 0).all()
    assert ((u[pos] & 0x80) == 0x80).all() and ((u[neg] & 0x80) == 0).all()
    assert len(np.unique(u)) == 256  # 0x7F too: the code of -1 .. -3


def test_pcm16_rounds_half_to_even_and_saturates():
    f = np.float32
    # k + 0.5 in units of 1/32767 is not representable in general: build the products instead, v * 32767 exactly k/2
    x = np.array([0.0, 1.0, -1.0, 1.5, -7.0, 0.99999, 1e-9, -1e-9], dtype=f)
    assert ao.pcm16_ref(x, 1.0).tolist() == [0, 32767, -32767, 32767, -32767, 32767, 0, 0]
    # exact halves: with gain 1/32767 * 32767 not exact, use the identity v * 32767 == s + 0.5 found by search
    s = np.arange(-40, 40, dtype=np.float64) + 0.5
    v = (s / 32767.0).astype(f)
    exact = (v * f(32767.0)).astype(np.float64) == s
    assert exact.sum() >= 8  # enough exact ties among them
    got = ao.pcm16_ref(v[exact], 1.0).astype(np.float64)
    assert (got % 2 == 0).all() and (np.abs(got - s[exact]) == 0.5).all()
    # the exhaustive grid s / 32767 comes back as s
    g = np.arange(-32767, 32768, dtype=np.int32)
    assert np.array_equal(ao.pcm16_ref((g / 32767.0).astype(f), 1.0), g.astype(np.int16))
    # gain is applied in fp32 before the clamp
    assert ao.pcm16_ref(np.array([0.25], dtype=f), 2.0).tolist() == [16384]  # 16383.5 -> even
    assert ao.pcm16_ref(np.array([0.75], dtype=f), 2.0).tolist() == [32767]


def test_gain_ref():
    assert ao.gain_ref(0.5, 0.01, None, 0.95) == np.float32(1.0)
    assert ao.gain_ref(0.5, 0.01, "peak", 0.95) == np.float32(0.95 / 0.5)
    assert ao.gain_ref(0.5, 0.01, "rms", 0.1, limit=True) == np.float32(1.0)
    assert ao.gain_ref(0.5, 0.0001, "rms", 0.1, limit=True) == np.float32(2.0)   # 10 limited to 1 / peak
    assert ao.gain_ref(0.5, 0.0001, "rms", 0.1, limit=False) == np.float32(10.0)
    for mode in ("peak", "rms"):
        assert ao.gain_ref(0.0, 0.0, mode, 0.95) == np.float32(1.0)  # silent or empty
    assert ao.gain_ref(0.3, 0.02, "peak", 0.95).dtype == np.float32
    with pytest.raises(ValueError):
        ao.gain_ref(0.5, 0.01, "loudness", 0.95)


def test_resample_tile_matches_the_kernel():
    from matcha_hip import runtime as rt
    src = open(os.path.join(REPO, "matcha-tts_amd", "csrc", "mt_audio.hip")).read()
    m = re.search(r"constexpr int RS_TN = (\d+);", src)
    assert m and int(m.group(1)) == rt.RESAMPLE_TILE
    m = re.search(r"constexpr int RS_MAX_FACTOR = (\d+);", src)
    assert m and int(m.group(1)) == ao.MAX_FACTOR


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from matcha_hip import runtime as rt
    L = rt.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused while its arguments are checked

    def resample(up, down, Lin=1000, Lout=None, half=100):
        Lout = -(-Lin * up // down) if Lout is None else Lout
        return L.mt_resample(p, 1, Lin, None, 1, p, half, up, down, p, Lout, p, p, 1 << 30, None)

    def last():
        return L.mt_last_error().decode()

    assert resample(1025, 441) != 0 and "1025/441" in last()
    assert resample(320, 1025) != 0 and "320/1025" in last()
    assert resample(0, 3) != 0 and "0/3" in last()
    assert resample(4, 2) != 0 and "lowest terms" in last()
    assert resample(320, 441, Lin=1000, Lout=725) != 0 and "Lout 725" in last() and "726" in last()
    assert L.mt_resample_workspace_bytes(100, 1025, 1) == 0 and "1025/1" in last()
    assert L.mt_resample_workspace_bytes(4410, 320, 441) == 4 * 320 * 28

    def encode(normalize=0, level=1.0, encoding=0):
        return L.mt_audio_encode(p, 1, 16, None, p, p, normalize, level, 1, encoding, p, None, None)

    assert encode(encoding=3) != 0 and "encoding 3" in last()
    assert encode(encoding=-1) != 0 and "encoding" in last()
    assert encode(normalize=3) != 0 and "normalisation mode 3" in last()
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert encode(normalize=1, level=bad) != 0 and "level" in last(), bad
    assert L.mt_audio_stats(p, 0, 16, None, p, p, p, 1 << 20, None) != 0 and "audio_stats" in last()


def test_audio_output_refuses_host_tensors_and_bad_settings():
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    x = torch.zeros(2, 512)
    for kw in (dict(), dict(sample_rate=16000, normalize="peak", encoding="pcm16")):
        with pytest.raises(HipPathError):
            AudioOutput(**kw)(x)
    for fn in (lambda: rt.audio_stats(x), lambda: rt.encode_audio(x), lambda: rt.resample(x, None)):
        with pytest.raises(HipPathError):
            fn()
    with pytest.raises(ValueError):
        AudioOutput(sample_rate=22051)
    with pytest.raises(ValueError):
        AudioOutput(encoding="mp3")
    with pytest.raises(ValueError):
        AudioOutput(normalize="lufs")
    with pytest.raises(ValueError):
        AudioOutput(normalize="peak", level=0.0)
    o = AudioOutput(normalize="peak")
    assert o.level == 0.95
    assert AudioOutput(normalize="rms").level == pytest.approx(0.1)
