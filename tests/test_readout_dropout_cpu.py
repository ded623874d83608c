"""The readout's dropout on the fused paths without a GPU: the host mirror of the generator (tests/_philox.py) against
Philox4x32-10's published known-answer vectors, the mask convention, the new exports, the mode bit, the unchanged struct
layouts and the refusals that happen before anything is launched."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import _philox as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(REPO, "include", "molkgnn_hip.h")) as f:
        return f.read()


# Random123's known-answer vectors for philox4x32 with 10 rounds: (counter, key) -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_host_philox_matches_the_known_answer_vectors(counter, key, want):
    got = P.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == want


def test_philox_word_takes_word_element_mod_4_of_one_block():
    seed, offset = 0x0123456789ABCDEF, (7 << 32) | 11
    e0 = (1 << 62) + 40 * 32 + 8                     # 4-aligned: one block gives the four hidden units of a tail lane
    block = P.philox4x32_10((e0 >> 2, e0 >> 34, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    words = P.philox_word(seed, offset, np.arange(e0, e0 + 4, dtype=np.uint64))
    assert [int(w) for w in words] == [int(b) for b in block]


def test_keep_rule_matches_the_kernels_threshold_and_scale():
    words = np.array([0, 0xFF, 0x100, 0x33333300, 0x33333400, 0xFFFFFFFF], dtype=np.uint32)
    k = P.keep_scale(words, 0.2)
    u = (words >> 8).astype(np.float64) / 2 ** 24
    assert np.array_equal(k == 0, u < np.float32(0.2))
    assert np.all(k[k != 0] == np.float32(1.0) / np.float32(0.8))
    assert np.all(P.keep_scale(words, 0.0) == 1.0)


def test_readout_mask_is_a_function_of_the_atom_row_only():
    seed, offset, H = 987654321, 5, 32
    whole = P.readout_mask(seed, offset, 300, H, 0.2)
    for row0, n in ((0, 17), (17, 100), (117, 183)):                 # any chunking: the same rows
        assert np.array_equal(P.readout_mask(seed, offset, n, H, 0.2, row0=row0), whole[row0:row0 + n])
    padded = P.readout_mask(seed, offset, 307, H, 0.2)                 # appended padding atoms leave the real rows as they are
    assert np.array_equal(padded[:300], whole)
    frac = float((whole == 0).mean())
    n = whole.size
    assert abs(frac - 0.2) <= 5 * np.sqrt(0.2 * 0.8 / n), frac
    assert not np.array_equal(whole, P.readout_mask(seed, offset + 1, 300, H, 0.2))


def test_readout_and_head_elements_are_disjoint():
    # the head's elements mol * G + j stay below 2^62 for any batch the kernels take; the readout's start there, so the two
    # counters differ in their second word (element >> 34) and no draw is shared
    G, n_mols = 64, 1 << 31
    assert (n_mols * G) < P.READOUT_BASE
    e = np.array([P.READOUT_BASE], dtype=np.uint64)
    assert int(e[0] >> np.uint64(34)) == 1 << 28
    seed, offset = 42, 3
    head = P.head_mask(seed, offset, 64, 32, 0.5)
    ro = P.readout_mask(seed, offset, 64, 32, 0.5)
    assert not np.array_equal(head, ro)


def test_new_exports_are_declared_exported_and_typed():
    from molkgnn_amd import _lib
    assert _lib.ABI_VERSION == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    h = _header()
    for name in ("mkgnn_tail_fused_readout_dropout", "mkgnn_readout_dropout_mask"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(rf"\bint {name}\(", h), name
    assert re.search(r"int mkgnn_readout_dropout_mask\(const int64_t\* rng_pair, int64_t n_rows, int32_t H, float p, float\* keep,"
                     r"\s*int64_t keep_stride,\s*void\* stream\);", h)
    assert re.search(r"int mkgnn_tail_fused_readout_dropout\(const mkgnn_tail_args\* args, float readout_dropout_p,", h)


def test_mode_bit_and_struct_layouts():
    from molkgnn_amd import _lib
    m = re.search(r"#define\s+MKGNN_MOLECULE_READOUT_DROPOUT\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.MOLECULE_READOUT_DROPOUT == 32
    names = [f[0] for f in _lib.MoleculeNet._fields_]
    assert "reserved2" not in names
    i = names.index("readout_dropout")
    assert names[i - 1] == "head_dropout" and _lib.MoleculeNet._fields_[i][1] is ctypes.c_float
    # the readout dropout sits where reserved2 sat: the offsets of the C struct and of the ctypes one agree
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "molkgnn_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
           'sizeof(mkgnn_molecule_net), offsetof(mkgnn_molecule_net, head_dropout), offsetof(mkgnn_molecule_net, readout_dropout), '
           'offsetof(mkgnn_molecule_net, rng_state), sizeof(mkgnn_tail_args));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "off.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), os.path.join(d, "off.c"), "-o",
                        os.path.join(d, "off")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "off")], capture_output=True, text=True, check=True).stdout.split()]
    M = _lib.MoleculeNet
    assert got == [ctypes.sizeof(M), M.head_dropout.offset, M.readout_dropout.offset, M.rng_state.offset,
                   ctypes.sizeof(_lib.TailArgs)]
    assert M.readout_dropout.offset == M.head_dropout.offset + 4
    assert [f[0] for f in _lib.TailArgs._fields_][-2:] == ["defer_reduce", "loss_kind"]


def _last_error(lib) -> str:
    lib.mkgnn_last_error.restype = ctypes.c_char_p
    return (lib.mkgnn_last_error() or b"").decode()


def test_host_refusals_before_any_launch():
    from molkgnn_amd import _lib
    lib = _lib.load()
    pair = (ctypes.c_int64 * 2)(1, 2)
    keep = (ctypes.c_float * 64)()
    a = ctypes.addressof
    assert lib.mkgnn_readout_dropout_mask(None, 2, 32, 0.2, a(keep), 32, None) != 0
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert lib.mkgnn_readout_dropout_mask(a(pair), 2, 32, p, a(keep), 32, None) != 0, p
        assert "outside [0, 1)" in _last_error(lib)
    assert lib.mkgnn_readout_dropout_mask(a(pair), 2, 32, 0.2, a(keep), 16, None) != 0        # stride below H
    assert lib.mkgnn_readout_dropout_mask(a(pair), 0, 32, 0.2, a(keep), 32, None) == 0        # nothing to do, nothing launched
    assert lib.mkgnn_tail_fused_readout_dropout(None, 0.2, None, 0, None) != 0


def _net_and_batch(lib, _lib):
    st = _lib.MoleculeNet()
    st.num_layers, st.E = 3, 7
    F = 28
    for li in range(3):
        st.layer[li].F = F
        for d in range(4):
            st.layer[li].bank[d].num_kernels = (10, 20, 30, 50)[d]
        F = 110
    st.readout.F, st.readout.H, st.readout.G = F, 32, 32
    assert lib.mkgnn_molecule_supported(ctypes.byref(st), 28) == 1
    b = _lib.MoleculeBatch()
    b.n_atoms, b.n_mols, b.n_chunks, b.max_chunk_atoms = 40, 2, 1, 40
    fake = ctypes.c_int64(0)
    for nm in ("x", "chunk_mol_ptr", "mol_atom_ptr", "atom_degree", "atom_rank"):
        setattr(b, nm, ctypes.addressof(fake))                # (never read: the call is refused before)
    b.x_stride = 28
    return st, b, fake


@pytest.mark.parametrize("p,with_rng,message", [(1.0, True, "readout dropout outside [0, 1)"),
                                                (-0.5, True, "readout dropout outside [0, 1)"),
                                                (0.2, False, "readout dropout needs rng_state")])
def test_molecule_step_refuses_bad_readout_dropout(p, with_rng, message):
    from molkgnn_amd import _lib
    lib = _lib.load()
    st, b, fake = _net_and_batch(lib, _lib)
    pair = (ctypes.c_int64 * 2)(1, 2)
    st.readout_dropout = p
    st.rng_state = ctypes.addressof(pair) if with_rng else None
    emb = (ctypes.c_float * 64)()
    rc = lib.mkgnn_molecule_step(ctypes.byref(st), ctypes.byref(b), _lib.MOLECULE_READOUT_DROPOUT, None, None,
                                 ctypes.addressof(emb), None, None, None, 0, None)
    assert rc != 0 and message in _last_error(lib), _last_error(lib)
    # an unknown bit beyond it is still refused
    rc = lib.mkgnn_molecule_step(ctypes.byref(st), ctypes.byref(b), 64, None, None, ctypes.addressof(emb), None, None, None, 0, None)
    assert rc != 0 and "unknown mode bits" in _last_error(lib)


def test_readout_dropout_mask_refuses_a_host_pair_from_python():
    import torch
    from molkgnn_amd import readout as R
    with pytest.raises(Exception):
        R.readout_dropout_mask(torch.tensor([1, 2], dtype=torch.int64), 4, 32, 0.2)
    with pytest.raises(ValueError):
        R.readout_dropout_mask(torch.tensor([1, 2], dtype=torch.int64), 4, 32, 1.0)
