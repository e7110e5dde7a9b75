"""The seeded noise stream's CPU specification (matcha_hip/noise.py) and the argument checks of the seeded entry
points (CPU only: no kernel launches)."""
import itertools

import numpy as np
import pytest
import torch

from matcha_hip.noise import philox4x32_10, reference_noise, seed_key

SEEDS = (0, 1, 2 ** 63 - 1, -1)
T_MOM = 1024


@pytest.fixture(scope="module")
def streams():
    """reference_noise of SEEDS at T = 1024, computed once and read-only"""
    out = {s: reference_noise(s, T_MOM) for s in SEEDS}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Random123's known-answer vectors for Philox4x32-10"""
    got = philox4x32_10(counter, key)
    assert all(g.dtype == np.uint32 for g in got)
    assert " ".join(f"{int(g):08x}" for g in got) == want


def test_philox_broadcasts_counters():
    """array counters give, element for element, what the scalar calls give"""
    t = np.arange(5, dtype=np.uint64)[None, :]
    q = np.arange(3, dtype=np.uint64)[:, None]
    a = philox4x32_10((t, q, 0, 0), (7, 9))
    for qi, ti in itertools.product(range(3), range(5)):
        b = philox4x32_10((ti, qi, 0, 0), (7, 9))
        assert [int(w[qi, ti]) for w in a] == [int(w) for w in b]


def test_seed_key_is_the_twos_complement_halves():
    assert seed_key(0) == (0, 0)
    assert seed_key(-1) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert seed_key(2 ** 63 - 1) == (0xFFFFFFFF, 0x7FFFFFFF)
    assert seed_key(-2 ** 63) == (0, 0x80000000)
    assert seed_key(0x123456789) == (0x23456789, 0x1)


def test_stream_pins():
    """fix the key halves, the counter order (t, c // 4) and the cos / sin order"""
    a = reference_noise(0, 4)
    assert a.shape == (80, 4) and a.dtype == np.float64
    assert np.abs(a[:4, 0] - [0.99113748, -0.92466278, -0.61760905, -0.48206835]).max() < 1e-7
    b = reference_noise(1, 8)
    assert np.abs(b[:4, 5] - [-0.54052688, 1.83562479, -0.13882915, 2.12330997]).max() < 1e-7


def test_prefix_property(streams):
    for s in SEEDS:
        assert np.array_equal(reference_noise(s, 40), streams[s][:, :40])
    # fewer channels are a prefix too: the counter holds c // 4, not C
    assert np.array_equal(reference_noise(1, 40, C=8), streams[1][:8, :40])


def test_float32_evaluation_is_close(streams):
    """the same formula in numpy float32 on the same counters: the GPU parity test's yardstick"""
    r32 = reference_noise(0, T_MOM, dtype=np.float32)
    assert r32.dtype == np.float32
    assert np.abs(r32 - streams[0]).max() < 1e-5


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_moments(streams):
    """N = 81,920 values per seed, every bar five standard errors of the statistic under N(0, 1)"""
    N = 80 * T_MOM
    for s in SEEDS:
        x = streams[s]
        assert x.size == N
        m, v = x.mean(), x.var()
        kurt = ((x - m) ** 4).mean() / v ** 2
        lag_t, lag_c = _corr(x[:, :-1], x[:, 1:]), _corr(x[:-1], x[1:])
        print(f"seed {s}: mean {m:.4f} var-1 {v - 1:.4f} kurt-3 {kurt - 3:.4f} lag_t {lag_t:.4f} lag_c {lag_c:.4f}")
        assert abs(m) <= 5 / np.sqrt(N)
        assert abs(v - 1) <= 5 * np.sqrt(2 / N)
        assert abs(kurt - 3) <= 5 * np.sqrt(24 / N)
        assert abs(lag_t) <= 5 / np.sqrt(N)
        assert abs(lag_c) <= 5 / np.sqrt(N)
    for a, b in itertools.combinations(SEEDS, 2):
        c = _corr(streams[a], streams[b])
        assert abs(c) <= 5 / np.sqrt(N), (a, b, c)


def test_reference_noise_rejects_bad_shapes():
    with pytest.raises(ValueError):
        reference_noise(0, 8, C=6)
    with pytest.raises(ValueError):
        reference_noise(0, 0)


# ------------------------------------------------------------------ C ABI argument checks (before any HIP call)
def _err(L):
    return L.mt_last_error().decode()


def test_noise_fill_names_the_bad_argument():
    from matcha_hip import _lib
    L = _lib.lib()
    seeds = torch.zeros(2, dtype=torch.int64)  # host memory: never dereferenced, the checks come first
    z = torch.zeros(2 * 80 * 4)
    assert L.mt_noise_fill(None, None, 2, 80, 4, z.data_ptr(), None) != 0
    assert "seeds" in _err(L)
    assert L.mt_noise_fill(seeds.data_ptr(), None, 2, 78, 4, z.data_ptr(), None) != 0
    assert "C 78" in _err(L)
    assert L.mt_noise_fill(seeds.data_ptr(), None, 2, 80, 4, None, None) != 0
    assert "z is NULL" in _err(L)
    assert L.mt_noise_fill(seeds.data_ptr(), None, 2, 80, 0, z.data_ptr(), None) != 0
    assert "T 0" in _err(L)


def test_durations_scaled_names_the_bad_argument():
    from matcha_hip import _lib
    L = _lib.lib()
    a = torch.zeros(8)
    yl = torch.zeros(1, dtype=torch.int64)
    rc = L.mt_durations_scaled(a.data_ptr(), a.data_ptr(), None, 1, 8, a.data_ptr(), a.data_ptr(), yl.data_ptr(), None)
    assert rc != 0 and "length_scale" in _err(L)


def test_cfm_solve_seeded_names_the_bad_argument():
    from matcha_hip import runtime as rt
    eng = rt.DecoderEngine(160, 2, 1, 2, "fp32")
    L = rt.lib()
    a = torch.zeros(8)
    rc = L.mt_cfm_solve_seeded(eng.h, a.data_ptr(), None, None, a.data_ptr(), a.data_ptr(), None, 1, 4, 0, 1, 0,
                               a.data_ptr(), a.data_ptr(), 32, None)
    assert rc != 0 and "seeds" in _err(L)


# ------------------------------------------------------------------ Python argument handling (host tensors)
def test_seed_and_per_row_arguments():
    from matcha_hip import runtime as rt
    s = rt.seed_tensor([7, -3, 2 ** 63 - 1], 3, "cpu")
    assert s.dtype == torch.int64 and s.tolist() == [7, -3, 2 ** 63 - 1]
    assert rt.seed_tensor(torch.tensor([5, 6], dtype=torch.int32), 2, "cpu").dtype == torch.int64
    for bare in (7, np.int64(7), torch.tensor(7)):
        with pytest.raises(TypeError):
            rt.seed_tensor(bare, 1, "cpu")
    with pytest.raises(TypeError):
        rt.seed_tensor([0.5, 1.5], 2, "cpu")
    with pytest.raises(ValueError):
        rt.seed_tensor([1, 2], 3, "cpu")
    with pytest.raises(ValueError):
        rt.seed_tensor(torch.zeros(2, 2, dtype=torch.int64), 2, "cpu")
    assert rt.is_scalar(1.0) and rt.is_scalar(2) and rt.is_scalar(np.float32(0.5)) and rt.is_scalar(torch.tensor(0.5))
    assert not rt.is_scalar([0.5]) and not rt.is_scalar(torch.ones(1))
    p = rt.per_row(0.667, 3, "cpu", "temperature")
    assert p.dtype == torch.float32 and p.tolist() == [np.float32(0.667)] * 3
    assert rt.per_row([0.3, 1.0], 2, "cpu", "temperature").tolist() == [np.float32(0.3), 1.0]
    with pytest.raises(ValueError, match="length_scale"):
        rt.per_row(torch.ones(4), 3, "cpu", "length_scale")
