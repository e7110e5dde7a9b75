"""The window calculus of streaming delivery (matcha_hip/stream_plan.py) on the host, against the
fp64 oracle: the vocoder's reach is derived from the config and is exactly the halo a window needs; the denoiser's
windows reproduce the one-shot call on the samples the plan keeps; every stage's crops partition the utterance, no
step reads what earlier steps have not made final, and the resampler's ranges concatenate to the whole.
"""
import itertools

import numpy as np
import pytest
import torch

from hifigan.config import v1
from matcha_hip import audio_out as ao
from matcha_hip import stream_plan as sp
from oracle import matcha_oracle as O

RB2 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=32,
           resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])


def _weights(h, c0, seed):
    """a random folded fp64 state dict of the config's layer structure at initial width c0 (the reach does not depend
    on the width; 32 keeps the oracle quick)"""
    g = torch.Generator().manual_seed(seed)

    def w(*shape):
        fan = shape[1] * shape[2]
        return torch.randn(*shape, generator=g, dtype=torch.float64) * (1.5 / fan ** 0.5)

    def b(n):
        return torch.randn(n, generator=g, dtype=torch.float64) * 0.1

    sd = {"conv_pre.weight": w(c0, 80, 7), "conv_pre.bias": b(c0)}
    nk = len(h["resblock_kernel_sizes"])
    c = c0
    for i, k in enumerate(h["upsample_kernel_sizes"]):
        sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"] = w(c, c // 2, k), b(c // 2)
        c //= 2
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}."
            for m in range(len(rd)):
                if h["resblock"] == "1":
                    sd[p + f"convs1.{m}.weight"], sd[p + f"convs1.{m}.bias"] = w(c, c, rk), b(c)
                    sd[p + f"convs2.{m}.weight"], sd[p + f"convs2.{m}.bias"] = w(c, c, rk), b(c)
                else:
                    sd[p + f"convs.{m}.weight"], sd[p + f"convs.{m}.bias"] = w(c, c, rk), b(c)
    sd["conv_post.weight"], sd["conv_post.bias"] = w(1, c, 7), b(1)
    return sd


def test_reach_of_v1_is_13():
    assert sp.vocoder_reach(v1) == 13
    rows = sp.vocoder_reach_table(v1)
    assert rows[-1][2:] == (-13, 13)
    assert sp.vocoder_hop(v1) == 256


@pytest.mark.parametrize("name", ["v1", "resblock2"])
def test_reach_is_the_halo_a_window_needs(name):
    """fp64 oracle, T = 48: the interior block [16, 32) vocoded from a window with `reach` frames of halo equals the
    one-shot block (<= 1e-10); with reach - 1 frames it does not. A window that ends at the utterance's own start /
    end needs no halo there (the convs zero-pad at every layer there, as the one-shot call does). The second config
    (ResBlock2, three stages) has another reach: it is computed, not remembered."""
    h = dict(v1) if name == "v1" else RB2
    reach, hop = sp.vocoder_reach(h), sp.vocoder_hop(h)
    if name == "resblock2":
        assert hop == 256 and reach != 13
    sd = _weights(h, 32, 5)
    T = 48
    mel = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * 2.1 - 5.5
    full = O.generator_forward(sd, mel, h)[0, 0]
    assert full.shape == (T * hop,)

    def err(s, e, halo, lo=None, hi=None):
        ws = max(0, s - halo) if lo is None else lo
        we = min(T, e + halo) if hi is None else hi
        win = O.generator_forward(sd, mel[:, :, ws:we], h)[0, 0]
        return float((win[(s - ws) * hop:(e - ws) * hop] - full[s * hop:e * hop]).abs().max())

    e_in, e_short = err(16, 32, reach), err(16, 32, reach - 1)
    print(f"{name}: reach {reach}: halo reach {e_in:.2e}, halo reach - 1 {e_short:.2e}")
    assert e_in <= 1e-10
    assert e_short > 1e-10
    # one frame short on one side only: both ends of the interval are tight or the reach is the larger of the two
    lo, hi = sp.vocoder_interval(h, 0, hop - 1)
    assert max(-lo, hi) == reach
    if -lo == reach:
        assert err(16, 32, reach, lo=16 - reach + 1) > 1e-10
    if hi == reach:
        assert err(16, 32, reach, hi=32 + reach - 1) > 1e-10
    # true edges: no halo beyond the utterance
    assert err(0, 16, reach) <= 1e-10
    assert err(32, T, reach) <= 1e-10


def test_denoise_reach():
    assert sp.denoise_reach() == 4
    with pytest.raises(ValueError, match="odd frame"):
        sp.check_denoise_window(5, 12, 23)
    with pytest.raises(ValueError, match="odd frame"):
        sp.denoise_keep(3, 12, 23)
    assert sp.denoise_window(9, 16, 23)[0] % 2 == 0


def _stft_frame_sources(start, end, n):
    """brute force of stft_denoise2_kernel's index map: for every STFT frame g of the window [start, end) of an
    utterance of n hop blocks, whether its 1024 reflect-padded sample indices (as utterance positions) are those of
    frame start + g of the whole utterance"""
    Lw, Lg = 256 * (end - start), 256 * n

    def idx(f, L):
        i = f * 256 + np.arange(1024) - 512
        i = np.where(i < 0, -i, i)
        i = np.where(i >= L, 2 * (L - 1) - i, i)
        return np.clip(i, 0, L - 1)

    return [np.array_equal(idx(g, Lw) + 256 * start, idx(start + g, Lg)) for g in range(end - start + 1)]


@pytest.mark.parametrize("n", [1, 2, 3, 8, 23, 40])
def test_denoise_keep_against_the_kernel_index_map(n):
    """every window the plan can make: a kept hop block is the overlap-add of the same STFT frames as in the one-shot
    call, each of them reads the same samples, and so does its partner in the pair FFT (or both have none)"""
    for start in range(0, n + 1, 2):
        for end in range(start + 1, n + 1):
            same = _stft_frame_sources(start, end, n)
            wl = end - start
            lo, hi = sp.denoise_keep(start, end, n)
            for J in range(lo, hi):
                j = J - start
                loc = list(range(max(0, j - 1), min(j + 2, wl) + 1))
                glo = list(range(max(0, J - 1), min(J + 2, n) + 1))
                assert [start + g for g in loc] == glo, (start, end, J)
                for g in loc:
                    assert same[g], (start, end, J, g)
                    mate = g ^ 1
                    has_l, has_g = mate <= wl, (start + mate) <= n
                    assert has_l == has_g and (not has_l or same[mate]), (start, end, J, g)


@pytest.mark.parametrize("n", [3, 8, 23])
@pytest.mark.parametrize("chunk", [5, 8])
def test_denoise_windows_against_oracle(n, chunk):
    """oracle.denoise in fp64 on each window of the plan (vocoder reach 0, so that the denoiser's windows follow the
    schedule closely): the kept samples are the one-shot call's to 1e-10 and the crops partition the utterance. (The
    fp64 oracle has no pair FFT: the GPU test with an odd chunk size checks the alignment's bits.)"""
    g = torch.Generator().manual_seed(n * 10 + chunk)
    audio = (torch.randn(1, n * 256, generator=g, dtype=torch.float64) * 0.3).clamp(-1, 1)
    bias = torch.rand(1, 513, 1, generator=g, dtype=torch.float64)
    ref = O.denoise(audio, bias, 0.5)[0]
    pl = sp.plan([n], chunk, reach=0)
    got = torch.full((n * 256,), float("nan"), dtype=torch.float64)
    covered = 0
    for st in pl.steps:
        for s, ln, lo, hi in zip(st.den.start, st.den.length, st.den.crop_lo, st.den.crop_hi):
            assert s % 2 == 0 and s + ln <= st.raw_final[0] and lo == covered
            win = O.denoise(audio[:, s * 256:(s + ln) * 256], bias, 0.5)[0]
            got[lo * 256:hi * 256] = win[(lo - s) * 256:(hi - s) * 256]
            if s > 0:  # the block before the kept ones is not exact: the crop is not wider than it may be by luck
                assert (win[(s + 2 - s) * 256:(s + 3 - s) * 256] - ref[(s + 2) * 256:(s + 3) * 256]).abs().max() > 1e-10
            covered = hi
    assert covered == n
    err = float((got - ref).abs().max())
    print(f"n {n} chunk {chunk}: {len(pl.steps)} steps, max |d| {err:.2e}")
    assert err <= 1e-10


FACTORS = [(1, 1), (320, 441), (160, 441), (320, 147)]


def _half(up, down):
    return 0 if (up, down) == (1, 1) else ao.design_filter(up, down)[1]


@pytest.mark.parametrize("chunk,first", list(itertools.product([1, 5, 16, 32], [None, 4])))
@pytest.mark.parametrize("up,down", FACTORS)
@pytest.mark.parametrize("denoise", [True, False])
def test_plan_partitions(chunk, first, up, down, denoise):
    rng = np.random.RandomState(chunk * 7 + (first or 0) + up)
    lens = [0, 1] + [int(v) for v in rng.randint(2, 120, size=6)]
    rng.shuffle(lens)
    half, reach = _half(up, down), 13
    pl = sp.plan(lens, chunk, first, up, down, half, reach=reach, denoise=denoise)
    B = len(lens)
    assert pl.n_out == [ao.out_length(256 * n, up, down) for n in lens]
    v_done, d_done, m_done = [0] * B, [0] * B, [0] * B
    done_count = [0] * B
    e_prev = 0
    for c, st in enumerate(pl.steps):
        assert st.s == e_prev and st.e == st.s + (chunk if c or first is None else first)
        e_prev = st.e
        seen = set()
        for b, s, ln, lo, hi in zip(st.voc.rows, st.voc.start, st.voc.length, st.voc.crop_lo, st.voc.crop_hi):
            n = lens[b]
            assert b not in seen and lo == v_done[b] and lo < hi <= n
            seen.add(b)
            assert 0 <= s and s + ln <= min(n, st.e + reach), "causality: no mel frame at or past e_c + reach"
            assert s <= max(0, lo - reach) and (s + ln == n or s + ln >= hi + reach)
            v_done[b] = hi
        assert v_done == st.raw_final
        if denoise:
            seen = set()
            for b, s, ln, lo, hi in zip(st.den.rows, st.den.start, st.den.length, st.den.crop_lo, st.den.crop_hi):
                n = lens[b]
                assert b not in seen and lo == d_done[b] and lo < hi <= n
                seen.add(b)
                assert s % 2 == 0 and s + ln <= v_done[b], "reads only final vocoder output"
                klo, khi = sp.denoise_keep(s, s + ln, n)
                assert klo <= lo and hi <= khi
                d_done[b] = hi
        else:
            assert st.den is None
            d_done = list(v_done)
        assert d_done == st.den_final
        assert st.m_lo == (pl.steps[c - 1].m_hi if c else 0) and st.m_hi >= st.m_lo
        last = sp.resample_last_read(st.m_hi, up, down, half)
        for b, (off, cnt, done) in enumerate(st.out_counts(pl.n_out)):
            assert off == m_done[b] and cnt >= 0
            m_done[b] += cnt
            done_count[b] += int(done)
            assert (m_done[b] == pl.n_out[b]) == (done_count[b] == 1), "done with the row's last sample, once"
            if d_done[b] < lens[b]:
                assert m_done[b] == st.m_hi and last < 256 * d_done[b], "reads only final denoised samples"
    assert v_done == lens and d_done == lens
    assert m_done == pl.n_out
    assert done_count == [1] * B


def test_plan_refuses_nonsense():
    for kw in (dict(lengths=[-1], chunk_frames=4), dict(lengths=[3], chunk_frames=0),
               dict(lengths=[3], chunk_frames=4, first_chunk_frames=0), dict(lengths=[3], chunk_frames=4, up=2, down=4)):
        with pytest.raises(ValueError):
            sp.plan(reach=13, **kw)


@pytest.mark.parametrize("up,down", FACTORS[1:])
def test_resample_ranges_concatenate_to_the_whole(up, down):
    """resample_range_ref over the plan's ranges == resample_ref, exactly, with the samples the plan has not made
    final yet set to NaN at the time of each range"""
    h, half = ao.design_filter(up, down)
    lens = [37, 5, 0, 1]
    rng = np.random.RandomState(up)
    xs = [rng.randn(256 * n) * 0.3 for n in lens]
    refs = [ao.resample_ref(x, up, down, h, half) for x in xs]
    pl = sp.plan(lens, 5, 4, up, down, half, reach=13)
    got = [[] for _ in lens]
    for st in pl.steps:
        for b, x in enumerate(xs):
            part = x.copy()
            part[256 * st.den_final[b]:] = np.nan
            got[b].append(ao.resample_range_ref(part, up, down, h, half, st.m_lo, st.m_hi))
    for b, ref in enumerate(refs):
        y = np.concatenate(got[b])
        assert y.shape == ref.shape == (pl.n_out[b],)
        assert np.array_equal(y, ref), b
