"""Audio output stage on the GPU (csrc/mt_audio.hip): mt_resample, mt_audio_stats, mt_audio_encode
and hifigan.output.AudioOutput against the CPU specification matcha_hip/audio_out.py.

  - the resampler against resample_ref in fp64 on the fp32-rounded taps, within the forward error bound of an fp32
    FMA chain, |err| <= (N + 1) 2^-24 A max|x| (N taps per phase, A the largest sum |h| over a phase: derived from the
    taps, not measured), with utterance ends around the kernel's tile boundaries;
  - unit impulses return the fp32 taps BIT FOR BIT (a phase or offset error cannot hide in a tolerance);
  - every row of a padded batch equals the one-utterance call on its crop, bit for bit, whatever the padding holds;
  - peak exact, meansq to fp64 accuracy, gain / PCM16 / mu-law bit-equal to the reference functions;
  - Generator -> Denoiser -> AudioOutput end to end.
"""
import numpy as np
import pytest
import torch

from conftest import make_generator

from matcha_hip import audio_out as ao

pytestmark = pytest.mark.gpu
DEV = "cuda"
SRC = 22050
# 320/441, 160/441 (the longest phase: 56 taps), 320/147, 2/1 and 1/2 (the shortest tables)
DSTS = {16000: (320, 441), 8000: (160, 441), 48000: (320, 147), 44100: (2, 1), 11025: (1, 2)}


def _plan(dst):
    from matcha_hip import runtime as rt
    plan = rt.resample_plan(SRC, dst)
    assert (plan.up, plan.down) == DSTS[dst]
    return plan


def _uniform(B, L, seed):
    return torch.rand(B, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).mul_(2).sub_(1).float()


def _bound(plan, xmax):
    P = np.abs(plan.taps_host.astype(np.float64))
    return (P.shape[1] + 1) * 2.0 ** -24 * P.sum(axis=1).max() * xmax


def _check_against_ref(plan, x, lens):
    """x [B, L] host fp32, lens host ints (samples) -> the device result, checked row by row"""
    from matcha_hip import runtime as rt
    B, L = x.shape
    y, ol = rt.resample(x.to(DEV), plan, torch.tensor(lens))
    assert y.shape == (B, plan.out_length(L)) and y.dtype == torch.float32 and ol.dtype == torch.int32
    y, ol = y.cpu().numpy(), ol.cpu().tolist()
    h32 = plan.h.astype(np.float32).astype(np.float64)
    worst = 0.0
    for b in range(B):
        n = lens[b]
        assert ol[b] == ao.out_length(n, plan.up, plan.down), (b, ol[b])
        assert not y[b, ol[b]:].any(), b
        if n == 0:
            continue
        xb = x[b, :n].numpy()
        ref = ao.resample_ref(xb, plan.up, plan.down, h32, plan.half)
        err = np.abs(y[b, :ol[b]] - ref).max()
        bound = _bound(plan, np.abs(xb).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
    return y, worst


@pytest.mark.parametrize("dst", list(DSTS))
def test_resample_against_fp64_reference(dst):
    plan = _plan(dst)
    x = _uniform(4, 4096, seed=dst)
    y, worst = _check_against_ref(plan, x, [4096, 1, 0, 2049])
    print(f"{SRC}->{dst}: max err / bound {worst:.3f}, max|y| {np.abs(y).max():.3f}")
    assert np.abs(y).max() > 1.0  # the resampled noise overshoots full scale: the encoder's clamp has work to do


@pytest.mark.parametrize("dst", list(DSTS))
def test_unit_impulses_return_the_fp32_taps_bit_for_bit(dst):
    from matcha_hip import runtime as rt
    plan = _plan(dst)
    up, down, half = plan.up, plan.down, plan.half
    L = 3001
    pos = [0, L // 2, L - 1]
    x = torch.zeros(3, L)
    for b, k0 in enumerate(pos):
        x[b, k0] = 1.0
    y, ol = rt.resample(x.to(DEV), plan)
    n_out = ao.out_length(L, up, down)
    assert ol.cpu().tolist() == [n_out] * 3
    h32 = plan.h.astype(np.float32)
    assert np.array_equal(ao.polyphase(h32, half, up), plan.taps_host)
    for b, k0 in enumerate(pos):
        j = half + np.arange(n_out, dtype=np.int64) * down - k0 * up
        ok = (j >= 0) & (j <= 2 * half)
        want = np.where(ok, h32[np.clip(j, 0, 2 * half)], np.float32(0.0)).astype(np.float32)
        assert ok.any()
        assert torch.equal(y[b].cpu(), torch.from_numpy(want)), (dst, k0)


@pytest.mark.parametrize("dst", list(DSTS))
def test_utterance_ends_around_tile_boundaries(dst):
    from matcha_hip import runtime as rt
    plan = _plan(dst)
    Tn = rt.RESAMPLE_TILE
    targets = [Tn - 1, Tn, Tn + 1, 2 * Tn + 1]
    lens = [(t - 1) * plan.down // plan.up + 1 for t in targets]  # the shortest utterance with at least t outputs
    n_outs = [ao.out_length(n, plan.up, plan.down) for n in lens]
    if plan.up <= plan.down:  # every output count is reachable when the rate goes down
        assert n_outs == targets
    else:                     # going up they come in steps of up / down: the first count at or past the target
        assert all(0 <= n - t < -(-plan.up // plan.down) for n, t in zip(n_outs, targets))
    x = _uniform(4, max(lens) + 3, seed=7 + dst)
    _, worst = _check_against_ref(plan, x, lens)
    print(f"{SRC}->{dst}: n_out {n_outs}, max err / bound {worst:.3f}")


def _pipeline(x, lens, plan, normalize, level, limit):
    """resample -> stats -> gain -> the three encodings; lens in samples or None"""
    from matcha_hip import runtime as rt
    y, ol = rt.resample(x, plan, lens)
    peak, meansq = rt.audio_stats(y, ol)
    outs = {}
    for enc in ao.ENCODINGS:
        outs[enc], gain = rt.encode_audio(y, ol, normalize, level, limit, enc, stats=(peak, meansq))
    return y, ol, peak, meansq, gain, outs


@pytest.mark.parametrize("normalize,limit", [("peak", True), ("rms", True), ("rms", False)])
def test_rows_do_not_depend_on_the_batch(normalize, limit):
    """Row b of a padded batch of five equals the one-utterance call on its own crop, bit for bit: resampled samples,
    peak, meansq, gain and the three encodings; at two paddings (the padding holds other data each time) and with the
    rows permuted."""
    plan = _plan(16000)
    lens = [9000, 1, 0, 6100, 777]  # 9000 -> 6531 outputs: four resample tiles, two stats tiles
    base = _uniform(5, 9000, seed=21) * 0.4
    singles = {}
    for b, n in enumerate(lens):
        if n:
            singles[b] = _pipeline(base[b:b + 1, :n].contiguous().to(DEV), None, plan, normalize, None, limit)
    for L, perm in ((9000, [0, 1, 2, 3, 4]), (10234, [3, 2, 4, 0, 1])):
        x = _uniform(5, L, seed=L)  # what lies past an utterance's length must not matter
        for row, b in enumerate(perm):
            x[row, :lens[b]] = base[b, :lens[b]]
        pl = torch.tensor([lens[b] for b in perm], device=DEV)
        y, ol, peak, meansq, gain, outs = _pipeline(x.to(DEV), pl, plan, normalize, None, limit)
        for row, b in enumerate(perm):
            n = int(ol[row])
            assert n == ao.out_length(lens[b], plan.up, plan.down)
            if lens[b] == 0:
                assert float(peak[row]) == 0 and float(meansq[row]) == 0 and float(gain[row]) == 1
                continue
            y1, ol1, peak1, meansq1, gain1, outs1 = singles[b]
            assert int(ol1[0]) == n == y1.shape[1]
            assert torch.equal(y[row, :n], y1[0]), (L, b)
            assert torch.equal(peak[row], peak1[0]) and torch.equal(meansq[row], meansq1[0]), (L, b)
            assert torch.equal(gain[row], gain1[0]), (L, b)
            for enc in ao.ENCODINGS:
                assert torch.equal(outs[enc][row, :n], outs1[enc][0]), (L, b, enc)


def test_stats_and_gain():
    from matcha_hip import runtime as rt
    B, L = 5, 10001
    lens = [10001, 4097, 0, 5000, 4096]
    x = _uniform(B, L, seed=31) * 0.3
    x[3, :5000] = 0.0  # a silent utterance in front of loud padding
    xd = x.to(DEV)
    ld = torch.tensor(lens, device=DEV)
    peak, meansq = rt.audio_stats(xd, ld)
    assert peak.dtype == torch.float32 and meansq.dtype == torch.float64
    peak_h, meansq_h = peak.cpu().numpy(), meansq.cpu().numpy()
    for b, n in enumerate(lens):
        xb = x[b, :n].numpy()
        assert peak_h[b] == (np.abs(xb).max() if n else 0.0), b
        want = float((xb.astype(np.float64) ** 2).sum() / n) if n else 0.0
        # fp64 accumulation of exact squares: n roundings of 2^-53 each at the very worst, far inside 1e-9
        assert abs(meansq_h[b] - want) <= 1e-9 * want, (b, meansq_h[b], want)
    for normalize, level, limit in (("peak", None, True), ("peak", 0.5, True), ("rms", None, True),
                                    ("rms", 0.7, True), ("rms", 0.7, False), (None, None, True)):
        _, gain = rt.encode_audio(xd, ld, normalize, level, limit, "f32", stats=(peak, meansq))
        lv = rt.DEFAULT_LEVEL[normalize] if level is None else level
        want = np.array([ao.gain_ref(peak_h[b], meansq_h[b], normalize, lv, limit) for b in range(B)])
        assert np.array_equal(gain.cpu().numpy(), want), (normalize, level, limit, gain.cpu().numpy(), want)
        assert want[2] == 1.0 and want[3] == 1.0  # empty and silent rows
    # uniform noise of peak 0.3 has RMS 0.17: an RMS of 0.7 would clip, so the limit holds the gain at 1 / peak
    assert float(rt.encode_audio(xd, ld, "rms", 0.7, True, "f32")[1][0]) < float(
        rt.encode_audio(xd, ld, "rms", 0.7, False, "f32")[1][0])


@pytest.mark.parametrize("L", [4096, 4099])  # four samples per thread, and one (rows not 16-byte aligned)
def test_encodings_equal_the_reference_functions(L):
    from matcha_hip import runtime as rt
    lens = [L, 1, 0, 2049]
    x = _uniform(4, L, seed=41) * 1.5  # |x| up to 1.5: the clamp works with and without gain
    xd, ld = x.to(DEV), torch.tensor(lens, device=DEV)
    for normalize, limit in ((None, True), ("peak", True), ("rms", False)):
        f32, gain = rt.encode_audio(xd, ld, normalize, None, limit, "f32")
        pcm, gain2 = rt.encode_audio(xd, ld, normalize, None, limit, "pcm16")
        mu, gain3 = rt.encode_audio(xd, ld, normalize, None, limit, "mulaw")
        assert torch.equal(gain, gain2) and torch.equal(gain, gain3)
        assert f32.dtype == torch.float32 and pcm.dtype == torch.int16 and mu.dtype == torch.uint8
        assert f32.shape == pcm.shape == mu.shape == (4, L)
        g = gain.cpu().numpy()
        for b, n in enumerate(lens):
            xb = x[b, :n].numpy()
            q = ao.pcm16_ref(xb, g[b])
            assert np.array_equal(f32[b, :n].cpu().numpy(), ao.f32_ref(xb, g[b])), (normalize, b)
            assert np.array_equal(pcm[b, :n].cpu().numpy(), q), (normalize, b)
            assert np.array_equal(mu[b, :n].cpu().numpy(), ao.mulaw_ref(q)), (normalize, b)
            # tails: digital silence in each encoding
            assert not f32[b, n:].any() and not pcm[b, n:].any() and bool((mu[b, n:] == 0xFF).all()), b
            if normalize == "peak" and n:
                assert int(pcm[b, :n].int().abs().max()) == int(np.rint(np.float32(0.95) * np.float32(32767))), b


def test_every_pcm16_value_round_trips():
    """x = s / 32767 for every s in [-32767, 32767] comes back as s in PCM16 and as mulaw_ref(s) in mu-law"""
    from matcha_hip import runtime as rt
    s = np.arange(-32767, 32768, dtype=np.int32)
    x = torch.from_numpy((s / 32767.0).astype(np.float32))[None].to(DEV)
    pcm, gain = rt.encode_audio(x, None, None, None, True, "pcm16")
    mu, _ = rt.encode_audio(x, None, None, None, True, "mulaw")
    assert float(gain[0]) == 1.0
    assert np.array_equal(pcm[0].cpu().numpy(), s.astype(np.int16))
    assert np.array_equal(mu[0].cpu().numpy(), ao.mulaw_ref(s.astype(np.int16)))


def test_generator_denoiser_audio_output_end_to_end():
    from hifigan.denoiser import Denoiser
    from hifigan.output import AudioOutput
    from matcha_hip import synthetic
    g = make_generator("bf16")
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], 8)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.to(DEV).eval()
    g.remove_weight_norm()
    den = Denoiser(g, mode="zeros")
    B, T = 3, 24
    lens = [24, 9, 16]
    ld = torch.tensor(lens, device=DEV)
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(9)) * 2.1 - 5.5).to(DEV)
    stage = AudioOutput(16000, normalize="peak", encoding="pcm16")
    d = den(g(mel, lengths=ld).squeeze(1), strength=0.00025, lengths=ld)
    out = stage(d, ld)
    assert out.sample_rate == 16000 and out.audio.dtype == torch.int16 and out.lengths.dtype == torch.int32
    assert out.audio.shape == (B, ao.out_length(T * 256, 320, 441)) and out.gain.shape == (B,)
    assert out.lengths.cpu().tolist() == [ao.out_length(256 * n, 320, 441) for n in lens]
    for b, n in enumerate(lens):
        one = stage(den(g(mel[b:b + 1, :, :n].contiguous()).squeeze(1), strength=0.00025))
        m = int(out.lengths[b])
        assert one.audio.shape == (1, m) and int(one.lengths[0]) == m
        assert torch.equal(out.audio[b, :m], one.audio[0]), b
        assert torch.equal(out.gain[b], one.gain[0]), b
        assert not out.audio[b, m:].any()
        assert int(out.audio[b, :m].int().abs().max()) == 31129  # rint(0.95 * 32767)
    # [B, 1, L] input; and the identity configuration is the reference's `.clamp(-1, 1)`, bit for bit
    ident = AudioOutput()(d.unsqueeze(1), ld)
    assert ident.sample_rate == 22050 and ident.audio.dtype == torch.float32
    assert torch.equal(ident.audio, d.clamp(-1, 1))
    assert ident.lengths.cpu().tolist() == [256 * n for n in lens] and bool((ident.gain == 1).all())
