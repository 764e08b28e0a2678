"""The reference's Link_prediction_model/negative_sample.py under its names and argument order, on the device samplers of ops.NegativeSampler
(csrc/cb_lpx.hip).  A graph.CSRGraph stands where the reference passes `edge_index`: "is (u, v) an edge" is a binary search in row v of its by-dst
CSR instead of PyG's linearise / sort / isin over the whole edge list.  Every result indexes like the reference's [num_samples, num_neg, 2] and is a
view of the sampler's int32 [2, S] storage (entry [i, j] = column i * num_neg + j).  `seed` (None: drawn from torch's CPU generator, so a run under
torch.manual_seed repeats) names the draws: the samplers are pure functions of it.  The sampler of a graph is kept on the graph; its failed-slot
counter is read by `check(graph)`, where the caller reads the loss anyway."""
import torch

from .. import ops


def sampler_of(graph):
    s = getattr(graph, '_lpx_sampler', None)
    if s is None:
        s = graph._lpx_sampler = ops.NegativeSampler(graph)
    return s


def check(graph):
    """Raises if a global draw on `graph` since the last check left a slot without a non-edge (one host read)."""
    sampler_of(graph).check()


def _as_reference(out, num_neg):
    """int32 [2, S] -> the view [S / num_neg, num_neg, 2]."""
    return out.t().view(-1, max(int(num_neg), 1), 2) if out.shape[1] else out.new_zeros((0, max(int(num_neg), 1), 2))


def global_neg_sample(graph, num_nodes, num_samples, num_neg, method='sparse', seed=None):
    """negative_sample.py:5-19.  `method` is PyG's and has no counterpart here.  Deviation: PyG returns fewer pairs than asked on a dense graph and
    the reference pads with repeats; here a slot that finds no non-edge in 64 tries holds -1 and check(graph) raises."""
    sampler = sampler_of(graph)
    _same_nodes(graph, num_nodes)
    return _as_reference(sampler.global_(num_samples, num_neg, seed), num_neg)


def global_perm_neg_sample(graph, num_nodes, num_samples, num_neg, method='sparse', seed=None):
    """negative_sample.py:21-26: num_samples global negatives and num_neg - 1 seeded permutations of them."""
    sampler = sampler_of(graph)
    _same_nodes(graph, num_nodes)
    return _as_reference(sampler.global_perm(num_samples, num_neg, seed), num_neg)


def local_neg_sample(pos_edges, num_nodes, num_neg, random_src=False, seed=None):
    """negative_sample.py:28-40 with random_src=False: [i, j] = (pos_edges[i, 0], a uniform node).  pos_edges: [P, 2] on the device."""
    if random_src:
        raise NotImplementedError('local_neg_sample(random_src=True) is not built: the device sampler copies the source column (random_src=False)')
    if not torch.is_tensor(pos_edges) or pos_edges.dim() != 2 or pos_edges.shape[1] != 2:
        raise ValueError('local_neg_sample: pos_edges must be a [P, 2] tensor')
    return _as_reference(ops.local_negatives(pos_edges.t(), num_nodes, num_neg, seed), num_neg)


def sample_perm_copy(edge_index, target_num_sample, num_perm_copy, seed=None):
    """negative_sample.py:42-57 for edge_index [2, n] on the device: [i, j] = copy j's pair i, copy 0 = edge_index (padded to target_num_sample with
    the pairs a seeded permutation puts first, where the reference pads with a host randperm), copy j >= 1 = copy 0 permuted by
    ops.seeded_permutation(target_num_sample, seed + j).  Deviation: the reference concatenates the copies before its reshape, so its [i, j] mixes
    them; here [:, j] is copy j, which is what global_perm_neg_sample's caller reads as "negative j of positive i"."""
    seed = ops.next_seed() if seed is None else int(seed)
    n, target = int(edge_index.shape[1]), int(target_num_sample)
    base = edge_index.to(torch.int32)
    if n < target:
        if n == 0:
            raise ValueError('sample_perm_copy: no pair to copy')
        extra = ops.seeded_permutation(n, seed, edge_index.device).long().repeat(-(-(target - n) // n))[:target - n]
        base = torch.cat([base, base[:, extra]], dim=1)
    elif n > target:
        raise ValueError(f'sample_perm_copy: {n} pairs for target_num_sample = {target} (the reference\'s reshape needs n <= target)')
    return _as_reference(ops.perm_copies(base.contiguous(), num_perm_copy, seed), num_perm_copy)


def _same_nodes(graph, num_nodes):
    if num_nodes is not None and int(num_nodes) != int(graph.N):
        raise ValueError(f'num_nodes = {num_nodes} but the graph has {graph.N} nodes')
