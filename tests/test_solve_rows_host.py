"""Per-utterance step counts in one CFM solve, the host side (CPU only: no kernel launches): mt_cfm_rows_plan, the
evaluation plan mt_cfm_solve_rows itself loops over, through ctypes, and runtime.cosine_grid / step_plan."""
import ctypes
import math

import pytest
import torch

EULER, MIDPOINT = 0, 1


def _plan(counts, solver, cap=64):
    from matcha_hip import runtime as rt
    L = rt.lib()
    n = (ctypes.c_int32 * max(len(counts), 1))(*counts)
    rows = (ctypes.c_int32 * max(cap, 1))(*([-7] * max(cap, 1)))
    S = L.mt_cfm_rows_plan(n, len(counts), solver, rows, cap)
    return S, list(rows[:max(S, 0)]), L.mt_last_error().decode()


def test_rows_plan_euler_and_midpoint():
    S, rows, _ = _plan([5, 5, 3, 1], EULER)
    assert S == 5 and rows == [4, 3, 3, 2, 2]
    S, rows, _ = _plan([5, 5, 3, 1], MIDPOINT)
    assert S == 10 and rows == [4, 4, 3, 3, 3, 3, 2, 2, 2, 2]
    assert _plan([1], EULER)[:2] == (1, [1])
    assert _plan([1], MIDPOINT)[:2] == (2, [1, 1])
    # the cost of a mixed solve: the sum of the counts, not B x the largest
    assert sum(_plan([5, 5, 3, 1], EULER)[1]) == 5 + 5 + 3 + 1
    # a cap of exactly S is enough
    assert _plan([5, 5, 3, 1], EULER, cap=5)[0] == 5


@pytest.mark.parametrize("counts,solver,cap,word", [
    ([3, 5], EULER, 64, "sorted"),       # an increasing pair
    ([2, 0], EULER, 64, ">= 1"),         # a count < 1
    ([], EULER, 64, "empty"),            # B = 0
    ([5, 5, 3, 1], EULER, 4, "cap"),     # cap too small
    ([5, 5, 3, 1], MIDPOINT, 9, "cap"),
])
def test_rows_plan_errors(counts, solver, cap, word):
    S, _, msg = _plan(counts, solver, cap)
    assert S < 0
    assert msg and word in msg, msg


def test_runtime_rows_plan_wrapper():
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    assert rt.rows_plan([5, 3, 3, 1]) == [4, 3, 3, 1, 1]
    assert rt.rows_plan([2, 1], "midpoint") == [2, 2, 1, 1]
    with pytest.raises(HipPathError, match="sorted"):
        rt.rows_plan([1, 2])


def test_rows_workspace_is_reported():
    from matcha_hip import runtime as rt
    eng = rt.DecoderEngine(160, 2, 1, 2, "bf16")
    L = rt.lib()
    plain = L.mt_cfm_workspace_bytes(eng.h, 4, 48, 5, EULER)
    rows = L.mt_cfm_rows_workspace_bytes(eng.h, 4, 48, 5, EULER)
    # every evaluation's time embedding per utterance and the two [S][B] tables on top of the shared-time solve's
    assert rows > plain + 2 * 5 * 4 * 4
    assert L.mt_cfm_rows_workspace_bytes(eng.h, 4, 48, 5, MIDPOINT) > rows
    assert L.mt_cfm_rows_workspace_bytes(eng.h, 0, 48, 5, EULER) == 0


def test_cosine_grid():
    from matcha_hip import runtime as rt
    g = rt.cosine_grid(4)
    assert g.dtype == torch.float32 and g.shape == (5,) and g.device.type == "cpu"
    want = torch.tensor([1.0 - math.cos(math.pi / 2 * i / 4) for i in range(5)], dtype=torch.float64)
    assert (g.double() - want).abs().max() <= 2.0 ** -24  # one fp32 rounding of a value in [0, 1]
    assert g[0] == 0 and g[-1] == 1
    assert bool((g[1:] > g[:-1]).all())
    assert rt.cosine_grid(1).tolist() == [0.0, 1.0]
    with pytest.raises(ValueError):
        rt.cosine_grid(0)


def test_step_plan_arguments():
    from matcha_hip import runtime as rt
    assert rt.step_plan(3, None, 2) == ([3, 3], None)
    assert rt.step_plan(torch.tensor([3, 5]), None, 2) == ([3, 5], None)
    counts, grids = rt.step_plan(None, rt.cosine_grid(4), 3)
    assert counts == [4, 4, 4] and all(torch.equal(g, rt.cosine_grid(4)) for g in grids)
    counts, grids = rt.step_plan([3, 1], [rt.cosine_grid(3), [0.0, 1.0]], 2)
    assert counts == [3, 1] and grids[1].tolist() == [0.0, 1.0]
    for bad in [dict(n_timesteps=[3, 5, 1], t_span=None),               # wrong length
                dict(n_timesteps=[3, 0], t_span=None),                  # a count < 1
                dict(n_timesteps=3, t_span=rt.cosine_grid(4)),          # disagreeing count
                dict(n_timesteps=None, t_span=[rt.cosine_grid(4)]),     # one grid for two rows
                dict(n_timesteps=None, t_span=[0.0, 0.5, 0.5, 1.0]),    # not strictly increasing
                dict(n_timesteps=None, t_span=[0.0, 0.5, 1.5]),         # outside [0, 1]
                dict(n_timesteps=None, t_span=[-0.1, 0.5]),
                dict(n_timesteps=None, t_span=torch.tensor([0.5])),     # no step
                dict(n_timesteps=None, t_span=None)]:
        with pytest.raises(ValueError):
            rt.step_plan(B=2, **bad)
