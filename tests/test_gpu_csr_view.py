"""GPU: the graph argument of the aggregation ABI as graph.CSRGraph._view fills it.  The two mistakes a view builder can make — one orientation's CSR
paired with the other orientation's hub plan, and a workspace still sized for the row width of an earlier call — show as wrong sums on a graph whose
two orientations have different plans, called with a narrow, then a wide, then a medium row width.  Features are small integers, so every sum is
exact in fp32 (and the rows exact in bf16) whatever the order: all comparisons are bit for bit against an int64 index_add_."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 333
HUBS = {10: 40, 77: 55, 150: 70, 222: 85, 300: 100}      # node -> extra in-edges


def _edges():
    """Non-symmetric: every node sends to (u + 1) % N and (3u + 5) % N; the hub nodes collect 40 .. 100 more in-edges from sources taken round-robin,
    so no node sends more than 4 edges."""
    u = torch.arange(N)
    src, dst = [u, u], [(u + 1) % N, (3 * u + 5) % N]
    k = 0
    for hub, extra in HUBS.items():
        src.append((torch.arange(extra) + k) % N)
        dst.append(torch.full((extra,), hub))
        k += extra
    return torch.stack([torch.cat(src), torch.cat(dst)])


@pytest.fixture(scope='module')
def case():
    from gnn_tail_generalization_amd.graph import CSRGraph
    ei = _edges()
    G = CSRGraph(ei.to(DEV), N, hub_threshold=8)
    assert not G.symmetric and int(G.out_degrees().max()) <= 4 and 40 <= int(G.in_degrees().max()) <= 110
    assert G._plan.n_hubs > 0 and G._plan_t.n_hubs == 0
    gen = torch.Generator().manual_seed(0)
    feats = {d: torch.randint(-3, 4, (N, d), generator=gen) for d in (40, 512, 256)}
    acc = torch.randint(-3, 4, (N, 256), generator=gen)

    def ref(d, transpose):      # by-dst CSR: out[v] = sum of h[u] over edges u -> v; transposed: out[u] = sum of h[v]
        rows, cols = (ei[0], ei[1]) if transpose else (ei[1], ei[0])
        return torch.zeros((N, d), dtype=torch.int64).index_add_(0, rows, feats[d][cols])
    refs = {(d, tr): ref(d, tr) for d in feats for tr in (False, True)}
    return G, feats, acc, refs


def test_view_pairs_each_orientation_with_its_own_plan(case):
    from gnn_tail_generalization_amd import _lib
    G = case[0]
    lib = _lib.load()
    for d in (40, 512, 256):
        fwd, rev = G._view(d), G._view(d, transpose=True)
        assert (fwd.rowptr, fwd.col, fwd.n_hubs, fwd.n_chunks) == (G.rowptr.data_ptr(), G.col.data_ptr(), G._plan.n_hubs, G._plan.n_chunks)
        assert (rev.rowptr, rev.col, rev.n_hubs, rev.n_chunks) == (G.rowptr_t.data_ptr(), G.col_t.data_ptr(), 0, 0)
        assert fwd.hub_rows == G._plan.hub_rows.data_ptr() and fwd.hub_chunk_ptr == G._plan.hub_chunk_ptr.data_ptr()
        assert fwd.ws_bytes == lib.cb_spmm_workspace_bytes(G._plan.n_chunks, d) > 0 and fwd.ws == G._ws.data_ptr() and G._ws.numel() >= fwd.ws_bytes
        assert (fwd.n_rows, fwd.n_edges, fwd.hub_threshold, fwd.col_flags) == (N, G.E, 8, 0)


def test_sums_are_exact_across_row_widths_orientations_and_dtypes(case):
    G, feats, acc, refs = case
    G._ws = None                                   # the first call below sizes the workspace for d = 40
    acc_dev = acc.to(DEV, torch.float32)
    for d in (40, 512, 256):                       # narrow first: a workspace kept from it is too small for the next width
        for dtype in (torch.float32, torch.bfloat16):
            h = feats[d].to(DEV, dtype)
            for tr in (False, True):
                got = G.spmm(h, transpose=tr)
                assert got.dtype == torch.float32 and torch.equal(got.cpu().long(), refs[d, tr]), (d, dtype, tr)
                if d == 256:                       # running sums: the fp32 and the bf16 branch of the merged entry
                    got = G.spmm(h, transpose=tr, acc_init=acc_dev.clone())
                    assert torch.equal(got.cpu().long(), refs[d, tr] + acc), (d, dtype, tr, 'acc_init')
