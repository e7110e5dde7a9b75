"""Multi-speaker training surface, host side (CPU only: no kernel launches)."""
import os
import re
from types import SimpleNamespace

from conftest import DEC, DP, ENC, REPO

NEW = ("mtt_bcast_cols", "mtt_segsum_cols", "mtt_segsum_cols_scratch_floats")


def test_lightning_module_multi_speaker_constructs_with_two_tables():
    """MatchaLightningModule(n_spks = 109) constructs on the CPU with the reference's two speaker tables
    (train_standalone.py:604-605): its own, registered before the model (state key spk_emb.weight, the first
    parameter), and the model's (model.spk_emb.weight), each [109, 64]."""
    import train_standalone as TS
    mod = TS.MatchaLightningModule(178, 109, 64, SimpleNamespace(**ENC), SimpleNamespace(**DEC),
                                   {"solver": "euler", "sigma_min": 1e-4}, SimpleNamespace(**DP),
                                   {"mel_mean": 0.0, "mel_std": 1.0})
    sd = mod.state_dict()
    assert tuple(sd["spk_emb.weight"].shape) == (109, 64)
    assert tuple(sd["model.spk_emb.weight"].shape) == (109, 64)
    assert sd["spk_emb.weight"].data_ptr() != sd["model.spk_emb.weight"].data_ptr()
    names = [n for n, _ in mod.named_parameters()]
    assert names[0] == "spk_emb.weight" and "model.spk_emb.weight" in names
    # the optimizer's index: the module-level table is the engine's, the model's own table maps to nothing
    idx = mod.configure_optimizers()._index()
    assert idx[0] == "spk_emb.weight" and idx[names.index("model.spk_emb.weight")] is None
    assert len([n for n in idx if n == "spk_emb.weight"]) == 1


def test_header_and_signature_table_name_the_speaker_primitives():
    """The public header declares the three new training functions and the ctypes table names them (their
    agreement symbol by symbol is tests/test_abi_host.py's job)."""
    from matcha_hip import _lib
    src = open(os.path.join(REPO, "include", "matcha_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mtt_\w+)\s*\(", src))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.SIGNATURES, n
