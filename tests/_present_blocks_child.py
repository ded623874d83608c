"""Child process of tests/test_present_blocks_gpu.py::test_library_switch_off_ignores_the_hint: started with MKGNN_GRAD_BLOCKS=0."""
import os

import torch


def main():
    assert os.environ.get("MKGNN_GRAD_BLOCKS") == "0"
    from molkgnn_amd import _lib, molecule
    from molkgnn_amd import functional as Fn
    from tests.test_present_blocks_gpu import _Case
    molecule._MODE = "0"                                  # the per-operator path
    assert Fn.GRAD_BLOCKS is False
    Fn.GRAD_BLOCKS = True                                 # the package's half on again: tags are set, hints are sent
    lib = _lib.load()
    real, sent = lib.mkgnn_backward_grad_blocks, []

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def mkgnn_backward_grad_blocks(self, present8, blocks):
            if present8 is not None:
                sent.append(1)
            return real(present8, blocks)
    Fn._lib.load = lambda: Spy()
    case = _Case(seed=71)
    tagged, seen = [], []
    mark = Fn.mark_grad_blocks
    Fn.mark_grad_blocks = lambda h, plan, blocks: (tagged.append(h), mark(h, plan, blocks))[1]
    case.after_forward = lambda: [h.register_hook(lambda g: seen.append(g.detach().clone())) for h in tagged]
    Fn.debug_poison_backward(True)
    n0 = Fn.debug_grad_blocks_launches()
    loss = case.step()
    got = case.results(loss)
    Fn.debug_poison_backward(False)
    masked = Fn.debug_grad_blocks_launches() - n0
    whole = sum(int(bool(torch.isfinite(g).all())) for g in seen)
    assert bool(torch.isfinite(got[1]).all()) and all(bool(torch.isfinite(v).all()) for v in got[2].values())
    print(f"hints sent {len(sent)}, masked launches {masked}, whole rows {whole}")


if __name__ == "__main__":
    main()
