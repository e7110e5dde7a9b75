"""Mel infill, the host side (CPU only: no kernel launches): the Python argument errors, which come before anything asks
for the GPU, and mt_cfm_infill_workspace_bytes / mt_cfm_solve_infill's own checks through ctypes, which come before
any launch (the device pointers the checks do not reach are null)."""
import ctypes

import pytest
import torch

from conftest import make_matcha

EULER, MIDPOINT = 0, 1
B, T = 4, 48


def _engine():
    from matcha_hip import runtime as rt
    return rt.DecoderEngine(160, 2, 1, 2, "bf16")


def _cpu_inputs():
    mu = torch.zeros(B, 80, T)
    mask = torch.ones(B, 1, T)
    return mu, mask, torch.zeros(B, 80, T), torch.zeros(B, 80, T), torch.zeros(B, T, dtype=torch.bool)


# ---------------------------------------------------------------- Python argument errors, before require_gpu
def test_solve_infill_argument_errors_come_before_the_gpu():
    eng = _engine()
    mu, mask, z, x1, keep = _cpu_inputs()
    args = (None, z, 1.0, mu, mask, None, 3)
    with pytest.raises(ValueError, match="come together"):
        eng.solve(*args, x1=x1)
    with pytest.raises(ValueError, match="come together"):
        eng.solve(*args, keep=keep)
    with pytest.raises(ValueError):
        eng.solve(*args, x1=x1[:, :79], keep=keep)          # 79 channels
    with pytest.raises(ValueError):
        eng.solve(*args, x1=x1[:3], keep=keep)              # B - 1 rows
    with pytest.raises(ValueError):
        eng.solve(*args, x1=x1, keep=torch.zeros(B, T + 1))  # keep [B, T + 1]
    with pytest.raises(ValueError):
        eng.solve(*args, x1=x1, keep=torch.zeros(B, 2, T))
    with pytest.raises(ValueError):
        eng.solve(*args, x1=x1, keep=keep, sigma_min=1.0)
    with pytest.raises(TypeError):
        eng.solve(*args, x1=x1.to(torch.int32), keep=keep)


def test_infill_args_accepts_bool_and_numeric_keep():
    from matcha_hip import runtime as rt
    x1 = torch.zeros(2, 80, 8)
    for keep in (torch.tensor([[0, 2, 0, 0, 1, 0, 0, 0]] * 2), torch.tensor([[0, .5, 0, 0, -1, 0, 0, 0]] * 2),
                 torch.tensor([[False, True, False, False, True, False, False, False]] * 2)[:, None]):
        x, k = rt.infill_args(x1, keep, 2, 80, 8)
        assert x is x1 and k.dtype == torch.uint8 and k.shape == (2, 8) and k.is_contiguous()
        assert k.tolist() == [[0, 1, 0, 0, 1, 0, 0, 0]] * 2
    assert rt.infill_args(None, None, 2, 80, 8) == (None, None)


def test_cfm_forward_and_synthesize_argument_errors_come_before_the_gpu():
    m = make_matcha(1, "fp32").eval()
    mu, mask, z, x1, keep = _cpu_inputs()
    with pytest.raises(ValueError, match="come together"):
        m.decoder(mu, mask, 3, x1=x1)
    with pytest.raises(ValueError):
        m.decoder(mu, mask, 3, x1=x1, keep=torch.zeros(B, T + 1))
    x, xl = torch.randint(1, 178, (2, 9)), torch.tensor([9, 7])
    mel = torch.zeros(2, 80, 20)
    with pytest.raises(ValueError, match="come together"):
        m.synthesize(x, xl, 2, infill_mel=mel)
    with pytest.raises(ValueError, match="come together"):
        m.synthesize(x, xl, 2, infill_keep=torch.zeros(2, 20))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, 2, infill_mel=mel[:, :79], infill_keep=torch.zeros(2, 20))  # 79 channels
    with pytest.raises(ValueError):
        m.synthesize(x, xl, 2, infill_mel=mel, infill_keep=torch.zeros(2, 21))
    with pytest.raises(ValueError):
        m.synthesize(x, xl, 2, infill_mel=mel[0], infill_keep=torch.zeros(2, 20))        # no batch dimension
    with pytest.raises(TypeError):
        m.synthesize(x, xl, 2, infill_mel=mel.long(), infill_keep=torch.zeros(2, 20))
    with pytest.raises(ValueError):
        m.synthesise(x, xl, 2, infill_mel=mel, infill_keep=torch.zeros(3, 20))


def test_edit_argument_errors_come_before_the_gpu():
    m = make_matcha(1, "fp32").eval()
    x_old = torch.tensor([[5, 6, 7, 8, 9, 10, 11, 12]])
    x_new = torch.tensor([[5, 6, 30, 31, 32, 9, 10, 11, 12, 0]])
    mel, ml = torch.zeros(1, 80, 16), torch.tensor([16])
    ok = dict(x_old=x_old, x_old_lengths=torch.tensor([8]), mel=mel, mel_lengths=ml, x_new=x_new,
              x_new_lengths=torch.tensor([9]), n_timesteps=2)
    with pytest.raises(ValueError, match="tails"):       # 3 tokens after the old span, 4 after the new one
        m.edit(spans=[(2, 5, 5)], **ok)
    x_bad = x_new.clone()
    x_bad[0, 7] = 99
    with pytest.raises(ValueError, match="differ"):      # the same count, another id in the tail
        m.edit(spans=[(2, 4, 5)], **dict(ok, x_new=x_bad))
    x_bad = x_new.clone()
    x_bad[0, 0] = 99
    with pytest.raises(ValueError, match="differ"):      # ... in the prefix
        m.edit(spans=[(2, 4, 5)], **dict(ok, x_new=x_bad))
    with pytest.raises(ValueError):                      # a span outside the text
        m.edit(spans=[(2, 9, 10)], **ok)
    with pytest.raises(ValueError):                      # one span per utterance
        m.edit(spans=[], **ok)
    with pytest.raises(ValueError):                      # the kept tokens keep their recorded durations
        m.edit(spans=[(2, 4, 5)], durations=torch.ones(1, 10, dtype=torch.int64), **ok)
    with pytest.raises(ValueError):
        m.edit(spans=[(2, 4, 5)], token_scale=torch.ones(1, 10), **ok)
    with pytest.raises(ValueError):
        m.edit(spans=[(2, 4, 5)], **dict(ok, mel=mel[:, :79]))


# ---------------------------------------------------------------- the C entry point and its workspace
def test_infill_workspace_is_reported():
    from matcha_hip import runtime as rt
    eng, L = _engine(), rt.lib()
    for solver in (EULER, MIDPOINT):
        rows = L.mt_cfm_rows_workspace_bytes(eng.h, B, T, 5, solver)
        infill = L.mt_cfm_infill_workspace_bytes(eng.h, B, T, 5, solver)
        assert infill >= rows + 2 * B * T * 80 * 4  # z0 and the transposed x1
        assert L.mt_cfm_infill_workspace_bytes(eng.h, B + 1, T, 5, solver) > infill
        assert L.mt_cfm_infill_workspace_bytes(eng.h, B, T + 2, 5, solver) > infill
    assert L.mt_cfm_infill_workspace_bytes(eng.h, 0, T, 5, EULER) == 0
    assert L.mt_cfm_infill_workspace_bytes(None, B, T, 5, EULER) == 0


def _call(eng, n_steps, grid=None, keep=1, x1=1, sigma_min=1e-4, solver=EULER):
    """mt_cfm_solve_infill with fake non-null device pointers (never dereferenced: every case fails a host check
    first) -> (rc, message)"""
    from matcha_hip import runtime as rt
    L = rt.lib()
    fake = ctypes.c_void_p(256)
    n = (ctypes.c_int32 * len(n_steps))(*n_steps)
    g = None if grid is None else (ctypes.c_float * len(grid))(*grid)
    rc = L.mt_cfm_solve_infill(eng.h, fake, fake, None, None, fake, fake, None, fake if x1 else None,
                               fake if keep else None, sigma_min, len(n_steps), T, 0, n, g, solver, fake, fake,
                               1 << 40, None)
    return rc, L.mt_last_error().decode()


def test_solve_infill_refuses_before_any_launch():
    eng = _engine()
    rc, msg = _call(eng, [3, 5, 1, 3])
    assert rc != 0 and "sorted" in msg, msg
    rc, msg = _call(eng, [2, 1], grid=[0.0, 0.5, 0.5, 0.0, 1.0, 0.0])
    assert rc != 0 and "increasing" in msg, msg
    rc, msg = _call(eng, [2, 1], grid=[0.0, 0.5, 1.0, 0.5, 0.25, 0.0])
    assert rc != 0 and "increasing" in msg and "row 1" in msg, msg
    rc, msg = _call(eng, [2, 1], grid=[0.0, 0.5, 1.5, 0.0, 1.0, 0.0])
    assert rc != 0 and "[0, 1]" in msg, msg
    rc, msg = _call(eng, [2, 1], keep=0)
    assert rc != 0 and "keep is NULL" in msg, msg
    rc, msg = _call(eng, [2, 1], x1=0)
    assert rc != 0 and "x1 is NULL" in msg, msg
    for s in (-0.1, 1.0):
        rc, msg = _call(eng, [2, 1], sigma_min=s)
        assert rc != 0 and "sigma_min" in msg, msg
    rc, msg = _call(eng, [2, 0])
    assert rc != 0 and ">= 1" in msg, msg
