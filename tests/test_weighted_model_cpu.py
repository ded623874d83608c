"""``train.GNNModel.loss`` never drops a batch's loss weights in silence: where it cannot take them it raises.  No GPU."""
import pytest
import torch


def test_a_cpu_batch_with_weights_raises_before_anything_runs():
    from molkgnn_amd.synthetic import make_batch
    from molkgnn_amd.train import GNNModel
    b = make_batch(4, seed=1)
    model = GNNModel().train()
    b.weight = torch.ones(4)
    with pytest.raises(ValueError, match="weights"):
        model.loss(b)
    del b.weight
    b.weight_table, b.weight_rows = torch.ones(8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="weights"):
        model.loss(b)
    b.weight_table = b.weight_rows = None                    # (cleared, as CompactStaticBatch.gather leaves a shard without weights)
    from molkgnn_amd._lib import MolKGNNLibraryError
    with pytest.raises(MolKGNNLibraryError):                 # (no weights: the model's own "no CPU path" as before)
        model.loss(b)
