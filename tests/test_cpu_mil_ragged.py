"""Host side of the ragged MIL `vit` forward: grouping of consecutive bags, packing / offsets, validation -- no kernels."""
import pytest
import torch

from stamp_amd import mil_core
from stamp_amd.mil_core import MAX_SOLO_TILES, group_bags, pack_bags


def test_group_bags_limits_and_order():
    assert group_bags([], 4, 1000) == []
    assert group_bags([10] * 10, 4, 10 ** 9) == [(0, 4), (4, 8), (8, 10)]
    # rows = tiles + one class token per bag: 3 bags of 9 tiles fill 30 rows exactly, the fourth starts a new group
    assert group_bags([9, 9, 9, 9], 64, 30) == [(0, 3), (3, 4)]
    # a bag whose rows alone exceed the row limit runs alone
    assert group_bags([5, 100, 5], 64, 50) == [(0, 1), (1, 2), (2, 3)]
    # too long to share: alone, neighbours keep their order
    assert group_bags([3, 40000, 4, 5], 64, 10 ** 9) == [(0, 1), (1, 2), (2, 4)]
    assert group_bags([3, 33000, 4], 64, 10 ** 9, max_shared=10 ** 6) == [(0, 1), (1, 2), (2, 3)]          # the class-row tail limit always holds
    assert group_bags([3, 8000, 4, 7936], 64, 10 ** 9, max_shared=7935) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert group_bags([MAX_SOLO_TILES, 1], 64, 10 ** 9) == [(0, 2)]
    with pytest.raises(ValueError):
        group_bags([1], 0, 10)
    with pytest.raises(ValueError):
        group_bags([1], 1, 0)


def test_group_bags_covers_every_bag_once():
    g = torch.Generator().manual_seed(0)
    lengths = [int(x) for x in torch.randint(1, 20000, (300,), generator=g)]
    for k, rows, shared in ((1, 10 ** 9, 32767), (7, 262144, 7935), (64, 65536, 32767)):
        groups = group_bags(lengths, k, rows, shared)
        assert [a for a, _ in groups] == [0] + [e for _, e in groups[:-1]] and groups[-1][1] == len(lengths)
        for a, e in groups:
            assert 1 <= e - a <= k
            if e - a > 1:
                assert sum(lengths[a:e]) + (e - a) <= rows and max(lengths[a:e]) <= shared


def test_pack_bags_offsets_and_validation():
    bags = [torch.randn(t, 8) for t in (3, 1, 5)]
    coords = [torch.rand(t, 2) for t in (3, 1, 5)]
    rb = pack_bags(bags, coords, n_feats=8, need_coords=True, device="cpu")
    assert rb.lengths == (3, 1, 5) and rb.n_bags == 3 and rb.total_tiles == 9 and rb.max_tiles == 5
    assert rb.offsets.dtype == torch.int32 and rb.offsets.tolist() == [0, 3, 4, 9]
    assert torch.equal(rb.feats, torch.cat(bags)) and torch.equal(rb.coords, torch.cat(coords))
    assert pack_bags([torch.randn(2, 4).half(), torch.randn(3, 4).half()], device="cpu").feats.dtype == torch.float16
    assert pack_bags([torch.randn(2, 4).half(), torch.randn(3, 4)], device="cpu").feats.dtype == torch.float32
    with pytest.raises(ValueError, match="empty"):
        pack_bags([torch.randn(2, 8), torch.randn(0, 8)], device="cpu")
    with pytest.raises(ValueError, match="features"):
        pack_bags([torch.randn(2, 8), torch.randn(2, 9)], device="cpu")
    with pytest.raises(ValueError, match="features"):
        pack_bags([torch.randn(2, 9)], n_feats=8, device="cpu")
    with pytest.raises(ValueError, match="coords"):
        pack_bags([torch.randn(2, 8)], need_coords=True, device="cpu")
    with pytest.raises(ValueError, match="coords"):
        pack_bags([torch.randn(2, 8)], [torch.rand(3, 2)], device="cpu")
    with pytest.raises(ValueError):
        pack_bags([torch.randn(2, 8, 1)], device="cpu")


def test_forward_ragged_refuses_training_and_grad():
    from stamp_amd.mil import VisionTransformer

    m = VisionTransformer(dim_output=2, dim_input=8, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=False)
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged([torch.randn(3, 8)])
    m.eval()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged([torch.randn(3, 8)])
    with torch.no_grad():
        with pytest.raises(ValueError):
            m.forward_ragged([torch.randn(0, 8)])
        with pytest.raises(RuntimeError, match="GPU"):
            m.forward_ragged([torch.randn(3, 8)])


def test_predict_bags_per_call_is_ignored_by_other_heads():
    from stamp_amd.deploy import predict_

    class _Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(8, 3)

        def forward(self, bags, coords=None, mask=None):
            return self.lin(bags.mean(1))

    torch.manual_seed(0)
    head = _Head()
    batches = [(torch.randn(1, n, 8), torch.zeros(1, n, 2), None, None) for n in (5, 9, 2, 4)]
    pids = ["a", "b", "c", "d"]
    base = predict_(head, batches, pids, task="classification", device="cpu")
    got = predict_(head, batches, pids, task="classification", device="cpu", bags_per_call=3)
    assert list(got) == pids and all(torch.equal(got[p], base[p]) for p in pids)
    with pytest.raises(ValueError):
        predict_(head, batches, pids, task="classification", device="cpu", bags_per_call=0)
    assert callable(mil_core.forward_infer_ragged)
