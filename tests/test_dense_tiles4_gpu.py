"""The relation-graph layer with FOUR 16-row tiles per wave (dense_order_layer_kernel<4>, ULTRA_DOL_TILES=4): one workgroup walks
four row tiles of a sample over one stream of B operands.  Per tile the conversion, the rounded product and the k-ordered matrix
instruction are those of the one-tile form, so every output must equal it BIT FOR BIT -- for tile counts that leave the last
workgroup 1, 2 or 3 live tiles, a last tile with fewer than 16 rows, exactly one full workgroup, and a graph too small for the form."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# tile counts 2 (ineligible: see the last test), 3 (ditto), 4, 4 (one full workgroup), 5, 7 and 30
ROW_COUNTS = [17, 33, 49, 64, 70, 100, 474]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _relation_like_graph(num_node, fill, seed, num_type=4, sparse_type=None):
    """Edges listed type block after type block (hh, tt, ht, th), each (row, col, type) at most once; `sparse_type` is present
    in every third row only."""
    g = torch.Generator().manual_seed(seed)
    blocks = []
    for t in range(num_type):
        mask = torch.rand(num_node, num_node, generator=g) < fill
        if t == sparse_type:
            mask[torch.arange(num_node) % 3 != 0] = False
        rc = mask.nonzero().t()
        blocks.append(torch.cat([rc, torch.full((1, rc.shape[1]), t)]))
    e = torch.cat(blocks, dim=1)
    return e[:2].contiguous(), e[2].contiguous()


def _operands(dev, N, bs, seed):
    from torch import nn
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, N, 64, generator=g).to(dev)
    rel = torch.randn(bs, 4, 64, generator=g).to(dev) * 0.1
    point = (torch.arange(bs).to(dev) * 3 % N, torch.randn(bs, 64, generator=g).to(dev))
    tensor_bnd = torch.randn(bs, N, 64, generator=g).to(dev)
    torch.manual_seed(1)
    lin, ln = nn.Linear(128, 64).to(dev), nn.LayerNorm(64).to(dev)
    return x, rel, point, tensor_bnd, lin, ln


def _both_cases(plan, ops):
    """Point boundary with LayerNorm, ReLU and residual; tensor boundary with none of the three."""
    x, rel, point, tensor_bnd, lin, ln = ops
    pair = (plan.fused_layer(rel, x, lin, layer_norm=ln, relu=True, residual=True, point=point),
            plan.fused_layer(rel, x, lin, layer_norm=None, relu=False, residual=False, boundary=tensor_bnd))
    assert all(o is not None for o in pair)
    return pair


def _run_forms(plan, ops, monkeypatch):
    monkeypatch.setenv("ULTRA_DOL_LEAN", "0")
    outs = {}
    for tiles in ("1", "4"):
        monkeypatch.setenv("ULTRA_DOL_TILES", tiles)
        outs[tiles] = _both_cases(plan, ops)
    return outs


@pytest.mark.parametrize("bs", [1, 5])
@pytest.mark.parametrize("N", ROW_COUNTS)
def test_four_row_tiles_per_wave_keep_the_one_tile_bits(dev, N, bs, monkeypatch):
    from ultra_amd.rspmm import Plan
    ei, et = _relation_like_graph(N, 0.97, seed=N)
    plan = Plan(ei, et, N, 4, exact_order=True)
    assert plan.dense is not None
    outs = _run_forms(plan, _operands(dev, N, bs, seed=N), monkeypatch)
    assert torch.equal(outs["1"][0], outs["4"][0]) and torch.equal(outs["1"][1], outs["4"][1])


def test_four_row_tiles_with_a_type_absent_in_some_rows(dev, monkeypatch):
    """Fill 0.5, and type 2 absent from two rows in three: zero adjacency bytes inside live tiles."""
    from ultra_amd.rspmm import Plan
    N = 70
    ei, et = _relation_like_graph(N, 0.5, seed=7, sparse_type=2)
    plan = Plan(ei, et, N, 4, exact_order=True)
    assert plan.dense is not None
    outs = _run_forms(plan, _operands(dev, N, 5, seed=11), monkeypatch)
    assert torch.equal(outs["1"][0], outs["4"][0]) and torch.equal(outs["1"][1], outs["4"][1])


def test_four_row_tiles_match_rspmm_plus_update(dev, monkeypatch):
    """The four-tile layer against order-kernel aggregate + torch's update (different product blocking: the tolerance of
    test_dense_order_layer_matches_rspmm_plus_update)."""
    from ultra_amd.rspmm import Plan
    N, bs = 70, 5
    ei, et = _relation_like_graph(N, 0.97, seed=N)
    x, rel, point, _, lin, ln = _operands(dev, N, bs, seed=N)
    monkeypatch.setenv("ULTRA_DOL_LEAN", "0")
    monkeypatch.setenv("ULTRA_DOL_TILES", "4")
    got = Plan(ei, et, N, 4, exact_order=True).fused_layer(rel, x, lin, layer_norm=ln, relu=True, residual=True, point=point)
    assert got is not None
    agg = Plan(ei, et, N, 4, exact_order=True, dense=False).forward(rel, x, point=point)
    with torch.no_grad():
        want = torch.relu(ln(lin(torch.cat([x, agg], dim=-1)))) + x
    scale = want.abs().max().item()
    assert (got - want).abs().max().item() <= 2e-5 * max(scale, 1.0)


@pytest.mark.parametrize("bs", [1, 5])
def test_a_graph_of_fewer_than_four_tiles_falls_back_to_one_tile(dev, bs, monkeypatch):
    """N = 40 (three tiles): ULTRA_DOL_TILES=4 is not eligible, the launcher runs one tile per workgroup: the same bits."""
    from ultra_amd.rspmm import Plan
    N = 40
    ei, et = _relation_like_graph(N, 0.97, seed=N)
    plan = Plan(ei, et, N, 4, exact_order=True)
    assert plan.dense is not None
    outs = _run_forms(plan, _operands(dev, N, bs, seed=N), monkeypatch)
    assert torch.equal(outs["1"][0], outs["4"][0]) and torch.equal(outs["1"][1], outs["4"][1])
