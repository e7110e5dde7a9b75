"""Long-form join, host side (CPU only: no kernel launches): the specification in matcha_hip/join.py
against its own rules, and the argument checks of the C ABI and of LongForm."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

from matcha_hip import join as jn


# ---- edges_ref ------------------------------------------------------------------------------------------------

def test_edges_first_and_last_sample_loud():
    x = np.zeros(10, np.float32)
    x[0] = 0.5
    assert jn.edges_ref(x, 10, 0.1, 0) == (0, 1)
    assert jn.edges_ref(x, 10, 0.1, 3) == (0, 4)
    x = np.zeros(10, np.float32)
    x[9] = -0.5
    assert jn.edges_ref(x, 10, 0.1, 0) == (9, 10)
    assert jn.edges_ref(x, 10, 0.1, 3) == (6, 10)
    x[2] = 0.2
    assert jn.edges_ref(x, 10, 0.1, 1) == (1, 10)
    assert jn.edges_ref(x, 9, 0.1, 1) == (1, 4)       # the loud sample at 9 lies past n: not read


def test_edges_threshold_is_inclusive_in_fp32():
    thr = np.float32(0.01)
    below = np.nextafter(thr, np.float32(0))
    x = np.zeros(8, np.float32)
    x[3] = thr
    assert jn.edges_ref(x, 8, float(thr), 0) == (3, 4)
    x[3] = -thr
    assert jn.edges_ref(x, 8, float(thr), 0) == (3, 4)
    x[3] = below
    assert jn.edges_ref(x, 8, float(thr), 0) == (0, 0)
    # the threshold is rounded to fp32 before the compare: 0.01 as a double lies above fl32(0.01)
    x[3] = thr
    assert float(thr) < 0.01 or float(thr) > 0.01
    assert jn.edges_ref(x, 8, 0.01, 0) == (3, 4)


def test_edges_silent_nan_empty_and_pad_clamp():
    x = np.full(16, 1e-4, np.float32)
    assert jn.edges_ref(x, 16, 1e-3, 5) == (0, 0)
    x[4] = np.nan                                      # a NaN is not loud
    assert jn.edges_ref(x, 16, 1e-3, 5) == (0, 0)
    x[5], x[7] = 1.0, -1.0
    assert jn.edges_ref(x, 16, 1e-3, 2) == (3, 10)
    assert jn.edges_ref(x, 16, 1e-3, 100) == (0, 16)   # the pad clamps at both ends
    assert jn.edges_ref(x, 9, 1e-3, 100) == (0, 9)
    assert jn.edges_ref(x, 0, 1e-3, 2) == (0, 0)       # n = 0
    assert jn.edges_ref(np.zeros(4, np.float32), 4, 0.0, 0) == (0, 4)   # thr = 0: every non-NaN sample is loud
    for bad in (dict(thr=-1.0, pad=0), dict(thr=float("nan"), pad=0), dict(thr=float("inf"), pad=0),
                dict(thr=0.1, pad=-1)):
        with pytest.raises(ValueError):
            jn.edges_ref(x, 16, **bad)


# ---- plan_ref -------------------------------------------------------------------------------------------------

def test_plan_one_segment_and_empty_document():
    dst, dl, bad = jn.plan_ref([0, 1], [5], [25], [99], 3, 4, 100)
    assert dst.tolist() == [3] and dl.tolist() == [3 + 20 + 4] and bad == 0 and dst.dtype == dl.dtype == np.int32
    # document 1 owns nothing: head + tail
    dst, dl, bad = jn.plan_ref([0, 1, 1, 2], [5, 0], [25, 10], [7, 7], 3, 4, 100)
    assert dst.tolist() == [3, 3] and dl.tolist() == [27, 7, 17] and bad == 0
    # edges are clamped: start into [0, L], end into [start, L]
    dst, dl, _ = jn.plan_ref([0, 2], [-5, 90], [30, 200], [0, 0], 0, 0, 100)
    assert dst.tolist() == [0, 30] and dl.tolist() == [40]
    dst, dl, _ = jn.plan_ref([0, 2], [50, 0], [20, 10], [0, 0], 0, 0, 100)   # end < start: empty
    assert dst.tolist() == [0, 0] and dl.tolist() == [10]


def test_plan_empty_segment_between_two_others_and_gap_clamp():
    # lengths 10, 0, 10: nothing can overlap an empty segment, so negative gaps round it become 0
    dst, dl, _ = jn.plan_ref([0, 3], [0, 0, 0], [10, 0, 10], [-4, -4, 0], 0, 0, 50)
    assert dst.tolist() == [0, 10, 10] and dl.tolist() == [20]
    dst, dl, _ = jn.plan_ref([0, 3], [0, 0, 0], [10, 0, 10], [5, 6, 0], 1, 2, 50)
    assert dst.tolist() == [1, 16, 22] and dl.tolist() == [34]
    # a gap more negative than half the shorter neighbour is clamped to it: lengths 10 and 7 -> at most 3
    dst, dl, _ = jn.plan_ref([0, 2], [0, 0], [10, 7], [-100, 0], 0, 0, 50)
    assert dst.tolist() == [0, 7] and dl.tolist() == [14]
    dst, dl, _ = jn.plan_ref([0, 2], [0, 0], [10, 7], [-3, -100], 0, 0, 50)   # the last segment's gap is ignored
    assert dst.tolist() == [0, 7] and dl.tolist() == [14]
    dst, dl, _ = jn.plan_ref([0, 2], [0, 0], [10, 7], [-2, 0], 0, 0, 50)
    assert dst.tolist() == [0, 8] and dl.tolist() == [15]


def test_plan_never_covers_a_sample_three_times():
    rng = np.random.default_rng(5)
    worst = 0
    for _ in range(300):
        S = int(rng.integers(1, 9))
        L = 24
        start = rng.integers(0, 8, S)
        end = start + rng.integers(0, 13, S)
        gap = rng.integers(-30, 4, S)
        cut = sorted(rng.integers(0, S + 1, int(rng.integers(0, 3))).tolist())
        doc_first = [0] + cut + [S]
        dst, dl, bad = jn.plan_ref(doc_first, start, end, gap, int(rng.integers(0, 3)), int(rng.integers(0, 3)), L)
        assert bad == 0
        for d in range(len(doc_first) - 1):
            cover = np.zeros(int(dl[d]) + 1, np.int64)
            for s in range(doc_first[d], doc_first[d + 1]):
                n = int(min(end[s], L) - start[s])
                assert dst[s] >= 0 and dst[s] + n <= dl[d]
                cover[dst[s]:dst[s] + n] += 1
            worst = max(worst, int(cover.max()))
            assert cover.max() <= 2
            assert (np.diff(dst[doc_first[d]:doc_first[d + 1]]) >= 0).all()   # what the kernel's binary search needs
    assert worst == 2   # the cases do overlap


def test_plan_bad_flag_at_lcap():
    args = ([0, 2], [0, 0], [40, 40], [10, 0], 5, 5, 64)
    dst, dl, bad = jn.plan_ref(*args, Lcap=100)
    assert dl.tolist() == [100] and bad == 0 and dst.tolist() == [5, 55]
    dst, dl, bad = jn.plan_ref(*args, Lcap=99)
    assert dl.tolist() == [99] and bad == 1 and dst.tolist() == [5, 55]
    dst, dl, bad = jn.plan_ref(*args, Lcap=50)     # clamped, nothing wraps
    assert dl.tolist() == [50] and bad == 1 and dst.tolist() == [5, 50]
    big = 2 ** 31 - 1
    dst, dl, bad = jn.plan_ref([0, 3], [0] * 3, [64] * 3, [big, big, 0], 0, 0, 64)
    assert bad == 1 and dl.tolist() == [1 << 30] and dst.tolist() == [0, 1 << 30, 1 << 30]
    with pytest.raises(ValueError):
        jn.plan_ref(*args, Lcap=(1 << 30) + 1)
    with pytest.raises(ValueError):
        jn.plan_ref([0, 1], [0], [1], [0], -1, 0, 4)


# ---- ramp and join_ref ----------------------------------------------------------------------------------------

def test_ramp_halves_sum_to_one_within_an_ulp():
    for fade in (1, 2, 3, 5, 64, 80, 110, 240, 1001):
        r = jn.ramp(fade)
        assert r.dtype == np.float32 and r.shape == (fade,)
        assert (np.diff(r) > 0).all() and 0 < r[0] and r[-1] < 1
        s = r.astype(np.float64) + r[::-1].astype(np.float64)
        # each half is rounded once: the larger is under 1 (error <= 2^-25), the smaller under 1/2 (<= 2^-26)
        assert np.abs(s - 1.0).max() <= 2.0 ** -24, fade
    assert jn.ramp(0).shape == (0,)
    with pytest.raises(ValueError):
        jn.ramp(jn.FADE_MAX + 1)


def test_constant_segments_crossfade_to_one():
    """Two segments of ones overlapped by exactly one fade: the sum across the overlap is 1 +- 2^-23. Each weight is
    the fp64 value rounded once, |error| <= 2^-25 (a value under 1); the products with 1.0f are exact; the first add
    (0 + w) is exact; the second add rounds a sum near 1, at most 2^-24 (half an ulp of values in [1/2, 2) is at most
    2^-24). Total: 2 * 2^-25 + 2^-24 = 2^-23."""
    for fade in (1, 4, 37, 80):
        n = 3 * fade + 5
        seg = np.ones((2, n), np.float32)
        start, end = [0, 0], [n, n]
        dst, dl, bad = jn.plan_ref([0, 2], start, end, [-fade, 0], 0, 0, n)
        assert dst.tolist() == [0, n - fade] and dl.tolist() == [2 * n - fade] and bad == 0
        out = jn.join_ref(seg, start, end, [0, 2], dst, dl, fade)
        assert out.shape == (1, 2 * n - fade) and out.dtype == np.float32
        assert np.array_equal(out[0, fade:n - fade], np.ones(n - 2 * fade, np.float32))
        assert np.abs(out[0, n - fade:n].astype(np.float64) - 1.0).max() <= 2.0 ** -23
        assert np.array_equal(out[0, :fade], jn.ramp(fade)) and np.array_equal(out[0, -fade:], jn.ramp(fade)[::-1])


def test_join_of_one_segment_without_fade_is_the_segment():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 50)).astype(np.float32)
    dst, dl, _ = jn.plan_ref([0, 1], [0], [50], [0], 0, 0, 50)
    out = jn.join_ref(x, [0], [50], [0, 1], dst, dl, 0)
    assert np.array_equal(out, x)
    # trimmed, with head and tail, into a longer row: zeros round the kept samples, which are never touched
    x[0, :7] = np.nan
    x[0, 40:] = np.nan
    dst, dl, _ = jn.plan_ref([0, 1], [7], [40], [0], 3, 4, 50)
    out = jn.join_ref(x, [7], [40], [0, 1], dst, dl, 0, Ld=64)
    assert dl.tolist() == [40] and out.shape == (1, 64)
    assert np.array_equal(out[0, 3:36], x[0, 7:40]) and not out[0, :3].any() and not out[0, 36:].any()


def test_short_segments_scale_the_ramp():
    table = jn.ramp(8)
    assert np.array_equal(jn.weights_ref(20, 8, table), np.concatenate([table, np.ones(4, np.float32), table[::-1]]))
    # len 6: F = 3, indices ((2 j + 1) 8) // 6 = 1, 4, 6
    assert np.array_equal(jn.weights_ref(6, 8, table), np.concatenate([table[[1, 4, 6]], table[[6, 4, 1]]]))
    assert np.array_equal(jn.weights_ref(3, 8, table), np.array([table[4], 1.0, table[4]], np.float32))
    assert np.array_equal(jn.weights_ref(1, 8, table), np.ones(1, np.float32))
    assert jn.weights_ref(0, 8, table).shape == (0,)
    assert np.array_equal(jn.weights_ref(5, 0, jn.ramp(0)), np.ones(5, np.float32))


# ---- C ABI and Python arguments -------------------------------------------------------------------------------

def test_tile_constants_match_the_kernel():
    from matcha_hip import runtime as rt
    src = open(os.path.join(REPO, "matcha-tts_amd", "csrc", "mt_join.hip")).read()
    for name, value in (("ED_TILE", rt.EDGES_TILE), ("JP_CHUNK", rt.JOIN_PLAN_CHUNK), ("JN_TILE", rt.JOIN_TILE),
                        ("JN_MAX_ROWS", rt.JOIN_MAX_ROWS)):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == value, name
    m = re.search(r"constexpr int JN_MAX_FADE = 1 << (\d+);", src)
    assert m and 1 << int(m.group(1)) == jn.FADE_MAX
    m = re.search(r"constexpr int JN_MAX_L = 1 << (\d+);", src)
    assert m and 1 << int(m.group(1)) == jn.LCAP_MAX


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from matcha_hip import runtime as rt
    L = rt.lib()
    assert L.mt_abi_version() == 1
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused while its arguments are checked

    def last():
        return L.mt_last_error().decode()

    def edges(S=2, Ln=100, thr=0.01, pad=4, audio=p, start=p, end=p, ws=p, ws_bytes=1 << 30):
        return L.mt_audio_edges(audio, S, Ln, None, thr, pad, start, end, ws, ws_bytes, None)

    assert edges(S=0) != 0 and "S 0" in last()
    assert edges(S=65536) != 0 and "S 65536" in last()
    assert edges(Ln=0) != 0 and "L 0" in last()
    assert edges(Ln=(1 << 30) + 1) != 0 and "audio_edges: S" in last()
    for a in ("audio", "start", "end"):
        assert edges(**{a: None}) != 0 and "null argument" in last(), a
    for thr in (-0.5, float("nan"), float("inf")):
        assert edges(thr=thr) != 0 and "threshold" in last(), thr
    assert edges(pad=-1) != 0 and "pad -1" in last()
    assert edges(ws=None) != 0 and "workspace" in last()
    assert edges(ws=ctypes.c_void_p(4104)) != 0 and "16-byte aligned" in last()
    need = L.mt_audio_edges_workspace_bytes(3, 2 * rt.EDGES_TILE + 1)
    assert need == 3 * 3 * 2 * 4   # two ints per tile
    assert edges(S=3, Ln=2 * rt.EDGES_TILE + 1, ws_bytes=need - 1) != 0 and "workspace too small" in last()
    assert L.mt_audio_edges_workspace_bytes(0, 100) == 0 and "S 0" in last()

    def plan(D=1, S=2, Ln=100, head=0, tail=0, Lcap=1 << 30, doc_first=p, start=p, end=p, gap=p, dst=p, doc_len=p,
             bad=p):
        return L.mt_join_plan(doc_first, D, start, end, gap, S, Ln, head, tail, Lcap, dst, doc_len, bad, None)

    for a in ("doc_first", "start", "end", "gap", "dst", "doc_len", "bad"):
        assert plan(**{a: None}) != 0 and "null argument" in last(), a
    assert plan(S=0) != 0 and "S 0" in last()
    assert plan(D=0) != 0 and "D 0" in last()
    assert plan(S=65536) != 0 and "join_plan: S" in last()
    assert plan(D=65536) != 0 and "join_plan: S" in last()
    assert plan(Ln=0) != 0 and "L 0" in last()
    assert plan(head=-1) != 0 and "head -1" in last()
    assert plan(tail=-2) != 0 and "tail -2" in last()
    assert plan(Lcap=(1 << 30) + 1) != 0 and "Lcap" in last()
    assert plan(Lcap=0) != 0 and "Lcap 0" in last()

    def join(S=2, Ln=100, D=1, fade=8, Ld=64, seg=p, start=p, end=p, doc_first=p, dst=p, doc_len=p, ramp=p, out=p):
        return L.mt_join(seg, S, Ln, start, end, doc_first, D, dst, doc_len, ramp, fade, out, Ld, None)

    for a in ("seg", "start", "end", "doc_first", "dst", "doc_len", "out"):
        assert join(**{a: None}) != 0 and "null argument" in last(), a
    assert join(S=0) != 0 and "S 0" in last()
    assert join(D=0) != 0 and "D 0" in last()
    assert join(Ln=0) != 0 and "L 0" in last()
    assert join(Ld=0) != 0 and "Ld 0" in last()
    assert join(Ld=(1 << 30) + 1) != 0 and "join: L" in last()
    assert join(fade=-1) != 0 and "fade -1" in last()
    assert join(fade=jn.FADE_MAX + 1) != 0 and "fade" in last()
    assert join(fade=8, ramp=None) != 0 and "without a ramp" in last()


def test_runtime_wrappers_refuse_host_tensors_and_bad_arguments():
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    x = torch.zeros(2, 16)
    with pytest.raises(HipPathError):
        rt.audio_edges(x, None, 0.01, 0)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(HipPathError):
        rt.join_plan(torch.tensor([0, 2], dtype=torch.int32), i32, i32, i32, 0, 0, 16)
    with pytest.raises(HipPathError):
        rt.join(x, i32, i32, torch.tensor([0, 2], dtype=torch.int32), i32, i32[:1], 0)


def test_longform_argument_refusals():
    from hifigan.longform import Document, LongForm
    from hifigan.output import AudioOutput
    from matcha_hip._lib import HipPathError
    out = AudioOutput(16000, loudness=-16, encoding="pcm16")
    lf = LongForm(None, None, None, out)
    assert (lf.pad, lf.fade, lf.head, lf.tail) == (320, 80, 0, 0) and lf.trim_db == -40.0 and lf.max_batch == 32
    assert LongForm(None, None, None, out, trim_db=None).trim_db is None
    assert Document._fields == ("audio", "lengths", "sample_rate", "gain", "segments")
    with pytest.raises(TypeError):
        LongForm(None, None, None, None)
    for kw in (dict(max_batch=0), dict(trim_db=1.0), dict(trim_db=float("nan")), dict(trim_pad_ms=-1.0),
               dict(fade_ms=-1.0), dict(head_ms=-1.0), dict(tail_ms=-0.1), dict(fade_ms=2000.0),
               dict(pause_ms=float("inf"))):
        with pytest.raises(ValueError):
            LongForm(None, None, None, out, **kw)
    s = torch.tensor([3, 4, 5])
    for docs in ([], [[]], "text", [s], [[s.float()]], [[s.reshape(1, 3)]], [[torch.zeros(0, dtype=torch.int64)]]):
        with pytest.raises(ValueError):
            lf(docs)
    docs = [[s, s, s], [s]]
    for seeds in ([1], [1, 2, 3], [1, -1], [1, 1 << 43], [1, 2.5], 7):
        with pytest.raises(ValueError):
            lf(docs, seeds=seeds)
    for pauses in ([[1.0, 2.0]], [[1.0], []], [[1.0, 2.0], [3.0]], [[1.0, float("nan")], []]):
        with pytest.raises(ValueError):
            lf(docs, pauses=pauses)
    with pytest.raises(ValueError):
        lf(docs, spks=[0])
    assert lf._gaps([[-5.0, 100.0], []], [0, 3, 4]) == [-80, 1600, 0, 0]
    assert lf._gaps(None, [0, 3, 3, 4]) == [4000, 4000, 0, 0]
    assert lf._sentence_seeds([3, 5], lf._flatten(docs)[0], 2) == [3 << 20, (3 << 20) | 1, (3 << 20) | 2, 5 << 20]
    # no CPU fallback: host tensors are refused once the arguments pass
    with pytest.raises(HipPathError):
        lf(docs, seeds=[1, 2])
