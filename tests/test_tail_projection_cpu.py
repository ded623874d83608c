"""The deferred projection's entry points and switch, without a GPU: they exist in the binding, the header declares them, the
switch table has the new field with its row in INTEGRATION.md, and ``mkgnn_tail_args`` is what it was."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(REPO, *parts), encoding="utf-8").read()


def test_entry_points_exist_in_the_binding_and_the_header():
    from molkgnn_amd import _lib
    header = _read("include", "molkgnn_hip.h")
    for name in ("mkgnn_tail_defer_projection", "mkgnn_debug_tail_projection_launches"):
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert _lib.ABI_VERSION == 8                                        # additive
    assert [f[0] for f in _lib.TailArgs._fields_][-2:] == ["defer_reduce", "loss_kind"]
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()                                               # (typed: load() raises on a missing export)
        assert lib.mkgnn_tail_defer_projection.argtypes is not None


def test_the_switch_table_is_complete():
    switches = _read("molkgnn_amd", "csrc", "kgnn_switches.h")
    assert re.search(r"int tail_project_in_prepass;", switches)
    assert 's.tail_project_in_prepass = number("MKGNN_TAIL_PROJECT_IN_PREPASS", 2)' in switches
    # every field of the struct is assigned from the environment or left at its zero on purpose (the two with `if` forms)
    body = switches[switches.index("struct Switches {"):switches.index("};", switches.index("struct Switches {"))]
    fields = re.findall(r"^\s+(?:bool|int|char|double)\s+(\w+)(?:\[\d+\])?;", body, flags=re.M)
    assert "tail_project_in_prepass" in fields
    for f in fields:
        assert re.search(r"s\.%s\b" % f, switches), f
    doc = _read("INTEGRATION.md")
    rows = re.findall(r"^\| `(MKGNN_[A-Z0-9_]+)` \|", doc, flags=re.M)
    assert rows.count("MKGNN_TAIL_PROJECT_IN_PREPASS") == 1
    assert set(re.findall(r'"(MKGNN_[A-Z0-9_]+)"', switches)) <= set(rows)


def test_only_the_convolutions_own_output_asks_for_the_projection():
    """``tail_loss`` asks for the deferred projection only for a ``sim`` that comes straight from a kernel convolution: a leaf (as
    the tail's own tests feed it) hands its gradient to AccumulateGrad, which must find it written."""
    import torch
    from molkgnn_amd import readout as R
    leaf = torch.zeros(4, 8, requires_grad=True)
    assert not R._sole_reader_is_the_convolution(leaf)
    assert not R._sole_reader_is_the_convolution(leaf * 2.0)
