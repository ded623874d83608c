"""The multi-output fused tail without a GPU: the two symbols, every refusal of ``mkgnn_tail_fused_labels`` before a launch, the
workspace size, and ``GNNModel.multi_output_tail`` on a CPU batch (the definition route, on or off)."""
import ctypes as C

import pytest
import torch

from tests import _label_training_child as LT

LS = (10, 20, 30, 50)
FAKE = 0x1000                      # a non-null address that a refused call never reads


def _lib_():
    from molkgnn_amd import _lib
    return _lib, _lib.load()


def _args(_lib, n_atoms=100, n_mols=8, n_loss=8, kind=0, H=32, G=32):
    """``mkgnn_tail_args`` with dummy pointers: complete enough to pass every check in front of the label checks."""
    a = _lib.TailArgs()
    a.sim, a.sim_stride = FAKE, 112
    for i, L in enumerate(LS):
        a.num_kernels[i] = L
    a.buckets = FAKE
    for f in ("in_rowptr", "in_col", "out_rowptr", "out_col", "mol_ptr", "atom_mol", "head_weight", "head_bias", "target", "loss",
              "grad_sim", "grad_lin1_weight", "grad_lin1_bias", "grad_lin2_weight", "grad_lin2_bias", "grad_head_weight",
              "grad_head_bias"):
        setattr(a, f, FAKE)
    a.n_atoms, a.n_mols, a.n_loss_mols = n_atoms, n_mols, n_loss
    r = a.readout
    r.F, r.H, r.G = 110, H, G
    r.lin1_weight = r.lin1_bias = r.lin2_weight = r.lin2_bias = FAKE
    a.grad_sim_stride, a.loss_kind = 112, kind
    return a


def _labels(_lib, T=9, source="labels", **over):
    t = _lib.TailLabels()
    t.n_tasks, t.pred, t.pred_stride = T, FAKE, T
    if source == "labels":
        t.labels, t.label_stride, t.n_label_rows = FAKE, T, 8
    else:
        t.task, t.n_task = FAKE, 8
    for k, v in over.items():
        setattr(t, k, v)
    return t


def test_the_symbols_are_exported_and_bound():
    _lib, lib = _lib_()
    for name in ("mkgnn_tail_labels_workspace_bytes", "mkgnn_tail_fused_labels"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.mkgnn_tail_fused_labels.restype is C.c_int and lib.mkgnn_tail_labels_workspace_bytes.restype is C.c_size_t
    assert lib.mkgnn_abi_version() == 8
    import re
    from pathlib import Path
    text = Path(__file__).resolve().parents[1].joinpath("include", "molkgnn_hip.h").read_text()
    assert re.search(r"int mkgnn_tail_fused_labels\(const mkgnn_tail_args\* args, float readout_dropout_p, const mkgnn_tail_labels\*", text)
    assert "typedef struct mkgnn_tail_labels {" in text


def test_workspace_bytes():
    _lib, lib = _lib_()
    for n_atoms, n_mols in ((100, 8), (90000, 4096), (1, 1)):
        for T in (1, 9, 32):
            got = lib.mkgnn_tail_labels_workspace_bytes(110, 32, 32, n_atoms, n_mols, T)
            assert got >= lib.mkgnn_tail_workspace_bytes(110, 32, 32, n_atoms, n_mols) > 0, (n_atoms, n_mols, T)
    for bad in ((110, 32, 32, 100, 8, 0), (110, 32, 32, 100, 8, 33), (110, 32, 32, 0, 8, 9), (110, 32, 32, 100, 0, 9),
                (110, 64, 32, 100, 8, 9), (110, 32, 48, 100, 8, 9), (110, 32, 32, 100, 8, -1)):
        assert lib.mkgnn_tail_labels_workspace_bytes(*bad) == 0, bad


def _call(lib, a, t, w=None, rp=0.0):
    return lib.mkgnn_tail_fused_labels(C.byref(a), rp, C.byref(t) if t is not None else None, C.byref(w) if w is not None else None,
                                       FAKE, 1 << 30, None)


def test_every_refusal_comes_before_a_launch():
    """Null or dummy pointers throughout: a call that got as far as a launch (or a read) would fault, not return."""
    _lib, lib = _lib_()
    err = lambda: _lib.last_error() if hasattr(_lib, "last_error") else lib.mkgnn_last_error().decode()
    assert _call(lib, _args(_lib), None) != 0
    for T in (0, -3, 33):                                     # T out of range
        assert _call(lib, _args(_lib), _labels(_lib, T=T)) != 0, T
        assert "tasks outside" in err()
    both = _labels(_lib)
    both.task, both.n_task = FAKE, 8
    assert _call(lib, _args(_lib), both) != 0 and "exactly one" in err()                      # both label sources
    neither = _labels(_lib)
    neither.labels = None
    assert _call(lib, _args(_lib), neither) != 0 and "exactly one" in err()                   # neither
    pw = _lib.LossWeights()
    pw.pos_weight = FAKE
    for kind in (1, 2):                                       # pos_weight with a squared-error kind
        assert _call(lib, _args(_lib, kind=kind), _labels(_lib), pw) != 0 and "pos_weight" in err()
    assert _call(lib, _args(_lib), _labels(_lib, label_stride=8)) != 0 and "stride" in err()   # strides below T
    assert _call(lib, _args(_lib), _labels(_lib, pred_stride=8)) != 0 and "stride" in err()
    a = _args(_lib, G=20)
    a.emb, a.emb_stride = FAKE, 16                            # ... below G
    assert _call(lib, a, _labels(_lib)) != 0 and "stride" in err()
    assert _call(lib, _args(_lib), _labels(_lib, pred=None)) != 0 and "null" in err()          # null outputs
    a = _args(_lib)
    a.loss = None
    assert _call(lib, a, _labels(_lib)) != 0 and "null" in err()
    a = _args(_lib)
    a.target = None                                           # the task source reads its labels from args->target
    assert _call(lib, a, _labels(_lib, source="task")) != 0 and "null" in err()
    assert _call(lib, _args(_lib), _labels(_lib, n_label_rows=7)) != 0 and "rows" in err()     # a matrix shorter than the loss rows
    assert _call(lib, _args(_lib), _labels(_lib, source="task", n_task=7)) != 0 and "rows" in err()
    assert _call(lib, _args(_lib), _labels(_lib, row_ids=FAKE, n_label_rows=0)) != 0 and "rows" in err()
    big = _args(_lib, n_atoms=1 << 30, n_mols=1 << 27, n_loss=1 << 27)
    assert _call(lib, big, _labels(_lib, T=32, n_label_rows=1 << 27)) != 0 and "2^31" in err()
    assert _call(lib, _args(_lib, kind=7), _labels(_lib)) != 0                               # what the tail itself refuses
    assert _call(lib, _args(_lib), _labels(_lib), rp=1.0) != 0
    a = _args(_lib, H=64)
    assert _call(lib, a, _labels(_lib)) != 0 and "outside the fused tail" in err()


def test_the_attribute_defaults_to_the_environment_and_off():
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import GNNModel
    import os
    assert GNNModel.multi_output_tail is None
    assert R._MULTI_TAIL is (os.environ.get("MKGNN_MULTI_TAIL", "0") == "1")
    assert R.tail_labels_supported(1) and R.tail_labels_supported(32) and not R.tail_labels_supported(33) and not R.tail_labels_supported(0)


class _Net(torch.nn.Module):
    """Stands in for the network (its kernels run on the GPU only): a fixed embedding, and what it was asked for."""

    def __init__(self, emb):
        super().__init__()
        self.emb, self.asked = torch.nn.Parameter(emb), []

    def forward(self, data, _tail=None):
        self.asked.append(_tail)
        return self.emb * 1.0


@pytest.mark.parametrize("on", [None, False, True])
def test_a_cpu_batch_takes_the_definition_route(on, monkeypatch):
    """Off, unset or on: a CPU batch with labels runs ``label_head_reference`` behind the network's embedding, as today -- the
    network is not asked for the tail, and the loss is the same bit for bit."""
    from molkgnn_amd import readout as R
    from molkgnn_amd.train import GNNModel
    torch.manual_seed(0)
    model = GNNModel(num_layers=1, task_dim=LT.T, dropout_ratio=0.0, ffn_dropout_rate=0.25).train()
    model.gnn_model = _Net(torch.randn(40, 32, generator=torch.Generator().manual_seed(2)))
    import types
    batch = types.SimpleNamespace(x=torch.zeros(3, 28), labels=LT.label_matrix(40, 8))
    seen = []
    real = R.label_head_reference
    monkeypatch.setattr(R, "label_head_reference", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    monkeypatch.setattr(R, "tail_labels_loss", lambda *a, **k: pytest.fail("the fused tail on a CPU batch"))
    monkeypatch.setattr(R, "label_head_loss", lambda *a, **k: pytest.fail("a kernel on a CPU batch"))
    model.multi_output_tail = None
    torch.manual_seed(11)
    want = model.loss(batch).detach().clone()
    model.multi_output_tail = on
    del seen[:], model.gnn_model.asked[:]
    torch.manual_seed(11)
    got = model.loss(batch)
    assert len(seen) == 1 and model.gnn_model.asked == [None]
    assert torch.equal(got.detach(), want) and bool(torch.isfinite(got.detach())) and float(got.detach()) > 0
    got.backward()
    assert bool(torch.isfinite(model.ffn.weight.grad).all()) and float(model.gnn_model.emb.grad.abs().max()) > 0
