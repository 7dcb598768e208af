"""The order in which MDETR's entry points stamp their stages (kernels.stamp records a name at its first stamp): encode, the sweep stages and encode_pairs
run the text branch, the backbone and the join as ONE sequence, forked or not, and functions.REJOIN is cleared behind every call -- also behind
one that raised inside the text branch.  The lists are read off the code as it was before the stages were folded into one helper each; this file
passed unchanged on that commit."""
import pytest
import torch

from test_gpu_zz_pair_train import _small_model

pytestmark = pytest.mark.gpu

TEXT = ["fwd.text.start", "fwd.text.end"]
IMAGE = ["fwd.backbone.start", "fwd.backbone.end"]


@pytest.fixture(scope="module")
def setup(dev):
    from toist_amd import harness
    model = _small_model(dev)[0].eval()
    samples, tok, pi, pc, _, _ = harness.synthetic_pair_batch(2, 2, [(0, 0), (1, 1)], height=64, width=96, tokens=6, seed=5, max_targets=0, device=dev)
    return model, samples, tok, pi, pc


def _names(monkeypatch, dev, call):
    """The names `call` stamped, in the order of their first stamps; REJOIN must be None behind it."""
    from toist_amd import functions, kernels
    stamps = {"buf": torch.zeros(16, dtype=torch.int64, device=dev), "names": []}
    monkeypatch.setattr(kernels, "STAMPS", stamps)
    with torch.no_grad():
        result = call()
    torch.cuda.synchronize()
    assert functions.REJOIN is None
    return stamps["names"], result


@pytest.mark.parametrize("overlap", ["on", "off"])
def test_entry_points_stamp_their_stages_in_one_order(dev, setup, monkeypatch, overlap):
    from toist_amd import engine
    model, samples, tok, pi, pc = setup
    monkeypatch.setattr(engine, "OVERLAP", overlap)
    fork = ["fwd.fork"] if overlap == "on" else []
    both = fork + TEXT + IMAGE + ["fwd.join"]
    assert _names(monkeypatch, dev, lambda: model.encode(samples, tok))[0] == both
    names, (state, text) = _names(monkeypatch, dev, lambda: model.sweep_stages(samples, tok))
    assert names == both
    assert _names(monkeypatch, dev, lambda: model.encode_pairs(samples, tok, pi, pc))[0] == both
    # the text stage alone stamps a join only behind a fork; the image stage alone never does
    assert _names(monkeypatch, dev, lambda: model.sweep_text(tok))[0] == fork + TEXT + (["fwd.join"] if fork else [])
    assert _names(monkeypatch, dev, lambda: model.sweep_images(samples))[0] == IMAGE
    # captions encoded earlier: no text branch, the join is still stamped
    assert _names(monkeypatch, dev, lambda: model.sweep_stages(samples, text))[0] == IMAGE + ["fwd.join"]
    assert _names(monkeypatch, dev, lambda: model.encode_pairs(samples, text, pi, pc))[0] == IMAGE + ["fwd.join"]


def test_rejoin_is_cleared_when_the_text_branch_raises(dev, setup, monkeypatch):
    from toist_amd import engine, functions
    model, samples, tok, pi, pc = setup
    monkeypatch.setattr(engine, "OVERLAP", "on")

    def broken(tokenized):
        assert functions.REJOIN is not None              # the branch was forked: its programs would rejoin the main stream in backward
        raise RuntimeError("text branch")

    monkeypatch.setattr(model.transformer, "encode_text", broken)
    with torch.no_grad(), pytest.raises(RuntimeError, match="text branch"):
        model.encode_pairs(samples, tok, pi, pc)
    torch.cuda.synchronize()
    assert functions.REJOIN is None
