"""The present-block masks of the index plan (``plan.present8``, ``plan.contrib_present8``; ``mkgnn_plan_present_blocks``) against
their definition (tests/_present_blocks_cases.masks_by_definition): the plain-torch construction here on the CPU, the HIP builder
with ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from tests import _present_blocks_cases as GB

NAMES = ["small_molecules", "atom_without_bonds", "hub_of_all_degrees", "chain", "padded"]


def _batch(name, dev=None):
    if name == "padded":
        return GB.padded_batch(dev)
    b = GB.batches()[name]
    return b if dev is None else b.to(dev)


def _check(b, plan, name):
    want8, want_rows = GB.masks_by_definition(b, plan)
    got8, got_rows = plan.present8, plan.contrib_present8
    assert got8.dtype == torch.int8 and got_rows.dtype == torch.int8
    assert got8.shape[0] == b.x.shape[0] and got_rows.shape[0] == plan.scatter[1].shape[0]
    assert np.array_equal(got8.cpu().numpy(), want8), name
    assert np.array_equal(got_rows.cpu().numpy(), want_rows), name
    if name == "hub_of_all_degrees":
        assert int(want8[0]) == 15                          # neighbours of all four degrees
    if name == "chain":
        assert set(want8[2:-2].tolist()) == {2}             # inner atoms: degree-2 partners only
        assert int(want8[1]) == 3 and int(want8[0]) == 2    # next to an end: a degree-1 and a degree-2 partner; the end itself
    if name == "atom_without_bonds":
        assert (want8 == 0).sum() == 2                      # the two single atoms: no edge ends in them


@pytest.mark.parametrize("name", NAMES)
def test_masks_from_plain_torch_match_the_definition(name):
    from molkgnn_amd.plan import plan_from_data
    b = _batch(name)
    _check(b, plan_from_data(b), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_masks_from_the_plan_builder_match_the_definition(name):
    from molkgnn_amd.plan import plan_from_data
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    b = _batch(name, torch.device("cuda:0"))
    plan = plan_from_data(b)
    assert plan.build_hip()
    _check(b, plan, name)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small_molecules", "padded"])
def test_masks_from_the_one_pass_builder_match_the_definition(name):
    """The other route to a plan: ``receptive_field.build_index_hip`` (``mkgnn_index_build``) makes ``present8`` with the index
    structures it hands to ``BatchPlan.adopt``."""
    from molkgnn_amd import receptive_field as RF
    from molkgnn_amd.plan import plan_from_lists
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    b = _batch(name, torch.device("cuda:0"))
    sizes = [int(getattr(b, f"selected_index_deg{d}").numel()) for d in range(1, 5)]
    rf, parts = RF.build_index_hip(b.x, b.p, b.edge_index, b.edge_attr, sizes)
    assert parts["present8"].dtype == torch.int8 and parts["present8"].shape[0] == b.x.shape[0]
    plan = plan_from_lists(b.x.shape[0], *[[rf[f"{nm}_deg{d}"] for d in range(1, 5)]
                                           for nm in ("p_focal", "nei_p", "nei_edge_attr", "selected_index", "nei_index")], b.edge_index)
    assert plan.adopt(parts) and plan._present8 is parts["present8"]
    _check(b, plan, name)
    torch.cuda.synchronize()
