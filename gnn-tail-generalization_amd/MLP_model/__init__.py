"""The Cold Brew student MLPs on the HIP path — drop-in for the reference's MLP_model/__init__.py:1-156 (StudentBaseMLP, BlockResMLP,
SEMLP): same constructor signatures, attribute names and state_dict keys, so a `seMLP` / `seMLP-part-1` checkpoint of either side loads
strict=True into the other.

Every `[Linear, LayerNorm, GELU, Dropout]` group of a getMLP stack (utils.py:885-908) runs as the MFMA GEMM + one row kernel
(ops.linear_ln_gelu_dropout), `h + block(x)` on cb_axpby_f32, `last_dropout` on cb_dropout_f32, part 2's input on the assembly kernel
around the top-K replacement (ops.semlp_part2_input).  Modules are built lazily as in the reference — on the CPU with torch's generator,
then moved: same-seed initial weights are bit-identical to the reference's.

GraphMLP (:158-208) is built as the reference's own public names — GraphMLP, get_neighbor_contrastive_loss, cosine_sim — on the fused
neighbour-contrastive loss (ops.neighbor_contrastive_loss, csrc/cb_ncloss.hip) and trained by trainer.train_graphMLP() through the
GraphMLPStudent holder below.

Not built (NotImplementedError names the reason): --train_which=GraphMLP routed through SEMLP.forward_part2 / trainer.main() (a follow-up,
DESIGN.md §0), has_NCloss, --SEMLP__include_part1out=0.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops, tuning
from ..utils import D, HipLinear, graphUtils

TOPK_KERNEL_MAX = 8      # cb_topk_replace_f32 keeps K <= 8 candidates per lane


def next_seed():
    """Dropout seed of the student's row stages: torch's CPU generator, as ops.next_seed — but a source of its own, so that wrapping
    ops.next_seed observes the teacher's draws only."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class StudentSequential(nn.Sequential):
    """nn.Sequential with getMLP's child indices ('0.weight', '1.weight', '4.bias', ...) whose forward runs each
    [Linear, LayerNorm, GELU, Dropout] group as GEMM + row kernel.  Device float32 matrices only: there is no eager path."""

    def forward(self, x):
        from .._lib import require_device
        require_device(x)
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.Linear) and i + 3 < len(mods) and isinstance(mods[i + 1], nn.LayerNorm) and isinstance(mods[i + 2], nn.GELU)
                    and mods[i + 2].approximate == 'none' and isinstance(mods[i + 3], nn.Dropout)):
                ln, p = mods[i + 1], mods[i + 3].p
                seed = next_seed() if (self.training and p > 0) else None
                x = ops.linear_ln_gelu_dropout(x, m.weight, m.bias, ln.weight, ln.bias, ln.eps, p, self.training, seed)
                i += 4
            elif isinstance(m, nn.Dropout):
                x = ops.dropout(x, m.p, self.training, seed=next_seed() if (self.training and m.p > 0) else None)
                i += 1
            elif isinstance(m, HipLinear):
                x = m(x)
                i += 1
            else:
                raise NotImplementedError(f'StudentSequential: no kernel for {type(m).__name__} at position {i}')
        return x


def getMLP(neurons, activation=nn.GELU, bias=True, dropout=0.1, last_dropout=False, normfun='layernorm'):
    """utils.py:885-908 for the student: same modules, same order of construction (so the same draws from torch's generator)."""
    if activation is not nn.GELU or normfun != 'layernorm':
        raise NotImplementedError('the student row kernel is LayerNorm + exact GELU (what the reference constructs everywhere)')
    if len(neurons) in [0, 1]:
        return nn.Identity()
    if len(neurons) == 2:
        return HipLinear(*neurons)
    layers = []
    n = len(neurons) - 1
    for i in range(n - 1):
        layers.extend([HipLinear(neurons[i], neurons[i + 1], bias=bias), nn.LayerNorm(neurons[i + 1]), activation(), nn.Dropout(dropout)])
    layers.append(HipLinear(neurons[n - 1], neurons[n], bias=bias))
    if last_dropout:
        layers.append(nn.Dropout(dropout))
    return StudentSequential(*layers)


class StudentBaseMLP(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        dim_model = None if args.StudentBaseMLP.dim_model == -1 else args.StudentBaseMLP.dim_model
        self.model = BlockResMLP(dims_in_out=args.StudentBaseMLP.dims_in_out, dim_model=dim_model,
                                 skip_conn_period=args.StudentBaseMLP.skip_conn_period, num_blocks=args.StudentBaseMLP.num_blocks)

    def forward(self, x, edge_index=None, mask=None):
        if mask is not None:
            x = x[mask]
        return self.model(x)

    def get_emb4linkp(self, x, edge_index, mask=None):
        return self.model(x)


class BlockResMLP(nn.Module):
    def __init__(self, dims_in_out, num_blocks, skip_conn_period=2, dim_hidden=None, dim_model=None, activation=nn.GELU, bias=True, dropout=0.1):
        super().__init__()
        self.dims_in_out = dims_in_out
        self.dim_model = dim_model or min(max(dims_in_out), 256)
        self.dim_hidden = dim_hidden or int(self.dim_model * 1.5) + 2
        self.num_blocks = num_blocks
        self.in_proj = nn.Identity() if self.dim_model == dims_in_out[0] else HipLinear(dims_in_out[0], self.dim_model)
        self.out_proj = nn.Identity() if self.dim_model == dims_in_out[1] else HipLinear(self.dim_model, dims_in_out[1])
        neurons = [self.dim_model] + [self.dim_hidden] * (skip_conn_period - 1) + [self.dim_model]
        self.blocks = nn.ModuleList([getMLP(neurons, activation=activation, bias=bias, dropout=dropout, last_dropout=True)
                                     for _ in range(self.num_blocks - 1)])
        self.blocks.append(getMLP(neurons, activation=activation, bias=bias, dropout=dropout, last_dropout=False))

    def forward(self, x):
        x = self.in_proj(x)
        for block in self.blocks:
            x = ops.axpby(1.0, x, 1.0, block(x))          # h + block(x)
        return self.out_proj(x)


class SEMLP(nn.Module):
    """Cold Brew's MLP (MLP_model/__init__.py:50-156)."""

    def __init__(self, args, data, teacherGNN):
        super().__init__()
        self.hidden_dim = 256
        self.args = args
        self.train_mask = data.train_mask
        self.test_mask = data.test_mask
        self.train_idx = data.train_idx
        self.test_idx = data.test_idx
        if self.args.batch_size > len(self.train_idx):
            print(f'\n\n    Batch size too large...\n Changing batch_size from {self.args.batch_size} to {len(self.train_idx)}!\n\n')
            self.args.batch_size = len(self.train_idx)
        self.has_NCloss = False
        self.adj_pow = None
        self.topK_2_replace = args.SEMLP_topK_2_replace
        if args.train_which == 'GraphMLP':
            raise NotImplementedError('GraphMLP is not built: it needs a sparse adjacency power and an N_b x N_b neighbour-contrastive loss '
                                      '(MLP_model/__init__.py:158-196), neither of which has a kernel here')
        if not args.SEMLP__downgrade_to_MLP and not args.SEMLP__include_part1out:
            raise NotImplementedError('--SEMLP__include_part1out=0 is not built: the reference indexes the already gathered batch a second '
                                      'time with node ids there (MLP_model/__init__.py:109) and only runs when those happen to be in range')
        # (an nn.Module teacher becomes a submodule, as in the reference: its tensors are part of the state_dict under `teacherGNN.` and of
        # self.parameters(); they never receive a gradient here, so the optimisers leave them alone)
        self.teacherGNN = teacherGNN
        self.part1 = None
        self.part2 = None
        self.alphas = nn.Parameter(torch.tensor([0.0001, 0.0001]), requires_grad=True)
        self.on_build = None      # optional callable(name, module) run right after a lazy build, before the optimiser is created
        self._idx = (None, None)

    def train(self, mode=True):
        """nn.Module.train for the student's own modules; the teacher keeps the mode its owner gave it (the hand-off draws the targets in
        train mode and the teacher is not run again, so the reference's cascade is unobservable there — here the trainer's teacher stays
        as the hand-off left it)."""
        teacher = self._modules.get('teacherGNN')
        was = teacher.training if teacher is not None else None
        super().train(mode)
        if teacher is not None:
            teacher.train(was)
        return self

    # -- lazy construction (reference :74-89, :111-126): on the CPU with torch's generator, then moved to args.device ----------------
    def _dim_model(self):
        return None if self.args.StudentMLP__dim_model == -1 else self.args.StudentBaseMLP.dim_model

    def _make_opt(self):
        self.opt = self.optfun(self.parameters(), lr=self.args.lr, weight_decay=self.args.weight_decay)

    def build_part1(self, se_dim):
        neurons_io = [self.args.num_feats, int(se_dim)]
        if self.args.SEMLP_part1_arch == 'residual':
            part1 = BlockResMLP(dims_in_out=neurons_io, dim_model=self._dim_model(), skip_conn_period=self.args.StudentBaseMLP.skip_conn_period,
                                num_blocks=self.args.StudentBaseMLP.num_blocks)
        else:
            nlayer = int(self.args.SEMLP_part1_arch[0])
            part1 = getMLP([neurons_io[0]] + [256] * (nlayer - 1) + [neurons_io[1]], dropout=self.args.dropout_MLP)
        self.part1 = part1.to(self.args.device)
        if self.on_build is not None:
            self.on_build('part1', self.part1)
        if getattr(self, 'optfun', None) is not None:
            self._make_opt()
        return self.part1

    def build_part2(self, dim_in):
        if self.args.train_which == 'StudentBaseMLP':
            part2 = BlockResMLP(dims_in_out=[self.args.num_feats, self.args.num_classes_bkup], dim_model=self._dim_model(),
                                skip_conn_period=self.args.StudentBaseMLP.skip_conn_period, num_blocks=self.args.StudentBaseMLP.num_blocks)
        else:
            part2 = getMLP([int(dim_in), 256, self.args.num_classes_bkup], dropout=self.args.dropout_MLP)
        self.part2 = part2.to(self.args.device)
        if self.on_build is not None:
            self.on_build('part2', self.part2)
        if getattr(self, 'optfun', None) is not None:
            self._make_opt()
        return self.part2

    # -- batches ----------------------------------------------------------------------------------------------------------------------
    def index_on_device(self, batch_idx, device):
        """int64 device copy of a host index array (np.random.choice's result); the last one is kept: the trainer's loss reads the rows the
        forward gathered."""
        if self._idx[0] is batch_idx and self._idx[1].device == device:
            return self._idx[1]
        idx = torch.as_tensor(np.asarray(batch_idx) if not torch.is_tensor(batch_idx) else batch_idx, dtype=torch.int64)
        if idx.dtype == torch.bool or idx.dim() != 1:
            raise ValueError('batch_idx must be a vector of node ids')
        idx = idx.to(device)
        self._idx = (batch_idx, idx)
        return idx

    def _gather(self, x, batch_idx):
        return ops.gather_rows_by_index(x, self.index_on_device(batch_idx, x.device))

    def forward_part1(self, x, edge_index=None, batch_idx=None):
        if self.has_NCloss:
            raise NotImplementedError('has_NCloss needs the sparse adjacency power of GraphMLP, which is not built')
        if self.part1 is None:
            # (the reference asks the teacher, whose get_se_dim runs a whole forward for the width: the targets the trainer attached say it too)
            se = getattr(self, 'teacherSE', None)
            self.build_part1(se.shape[1] if se is not None else self.teacherGNN.model.model.get_se_dim(x, edge_index))
        if batch_idx is not None:
            x = self._gather(x, batch_idx)
        return self.part1(x)

    def forward_part2(self, x, batch_idx=None, edge_index=None):
        if batch_idx is not None:
            x = self._gather(x, batch_idx)
        if self.args.SEMLP__downgrade_to_MLP:
            part2_in = x
        else:
            # the reference hands the gathered batch on with batch_idx in the edge_index slot (:103): part 1 does not index again
            part1_out = self.forward_part1(x, batch_idx).detach()
            self._check_k()
            part2_in = ops.semlp_part2_input(self.alphas, x, part1_out, self.teacherSE, self.topK_2_replace)
        if self.part2 is None:
            self.build_part2(part2_in.shape[-1])
        return self.part2(part2_in)

    def forward(self, x, edge_index=None):
        return

    def _check_k(self):
        if not 1 <= int(self.topK_2_replace) <= TOPK_KERNEL_MAX:
            raise NotImplementedError(f'SEMLP_topK_2_replace={self.topK_2_replace}: the top-K replacement kernel (cb_topk_replace_f32) '
                                      f'selects 1 <= K <= {TOPK_KERNEL_MAX} teacher rows')

    def replacement(self, le_guess, node_idx=None):
        """:143-156 for all rows at once: softmax-weighted mix of the K teacher embeddings with the largest inner product."""
        self._check_k()
        q = le_guess.detach()
        if node_idx is not None:
            q = q[torch.as_tensor(np.asarray(node_idx), device=q.device, dtype=torch.long)]
        return ops.se_topk_replace(q.to(self.teacherSE.device), self.teacherSE, int(self.topK_2_replace)).detach()


class GraphMLP(nn.Module):
    """GraphMLP (https://arxiv.org/abs/2106.04051) as the reference restates it (MLP_model/__init__.py:158-188): a [Linear, LayerNorm, GELU,
    Dropout(0.6), Linear] stack of width 256, a Linear head, and the neighbour-contrastive loss of the batch embeddings against the r-th
    power of the normalised adjacency.  Built in the reference's order on the CPU with torch's generator, then moved: same-seed weights are
    bit-identical; state_dict keys model.0.*, model.1.*, model.4.*, out_proj.*.
    Deviations: the loss is evaluated only while self.training (the reference also evaluates it in its eval forwards and never reads it
    there; here eval forwards leave .loss_NContrastive = None); a batch_idx entry beyond the power's node count raises ValueError (the
    reference: IndexError)."""

    def __init__(self, args, train_mask):
        super().__init__()
        self.dropout = 0.6          # reported in the paper (:162-163)
        self.hidden_dim = 256
        self.args = args
        self.model = getMLP([args.num_feats, self.hidden_dim, self.hidden_dim], dropout=self.dropout)
        self.out_proj = HipLinear(self.hidden_dim, args.num_classes_bkup)
        self.train_mask = train_mask
        self.train_idx = torch.where(self.train_mask == True)[0]      # noqa: E712  (:169)
        if self.args.batch_size > len(self.train_idx):
            print(f'\n\n    Batch size too large...\n Changing batch_size from {self.args.batch_size} to {len(self.train_idx)}!\n\n')
            self.args.batch_size = len(self.train_idx)
        self.adj_pow = None
        self.to(args.device)

    def power(self, edge_index):
        """The device form of A~^r, built on the host at the first call (normalize_adj -> sparse_power -> ops.SparsePower) and kept.  With
        tuning.T.power_on_device and the model on a GPU only normalize_adj stays on the host: the products and the transpose run on the device
        (ops.SparsePower.from_adjacency)."""
        if self.adj_pow is None:
            adj = graphUtils.normalize_adj(edge_index.detach().cpu())
            device = self.out_proj.weight.device
            if tuning.T.power_on_device and device.type == 'cuda':
                self.adj_pow = ops.SparsePower.from_adjacency(adj, self.args.graphMLP_r, device)
            else:
                self.adj_pow = ops.SparsePower(graphUtils.sparse_power(adj, self.args.graphMLP_r), device)
        return self.adj_pow

    def forward(self, x, edge_index=None, batch_idx=None):
        """x: the already gathered batch [B, F]; batch_idx: its node ids.  Returns utils.D with .emb [B, C] and .loss_NContrastive."""
        power = self.power(edge_index)
        z = self.model(x)
        info = D()
        info.loss_NContrastive = get_neighbor_contrastive_loss(z, power, batch_idx, self.args.graphMLP_tau) if self.training else None
        info.emb = self.out_proj(z)
        return info

    def get_emb4linkp(self, x, edge_index, mask=None):
        raise NotImplementedError


def get_neighbor_contrastive_loss(z, adj_pow, batch_idx, tau):
    """:190-198 on the fused kernels.  adj_pow: an ops.SparsePower, or a torch sparse tensor that is converted on every call."""
    if not isinstance(adj_pow, ops.SparsePower):
        adj_pow = ops.SparsePower(adj_pow, z.device)
    return ops.neighbor_contrastive_loss(z, adj_pow, batch_idx, tau)


def cosine_sim(x):
    """:200-208: pair-wise cosine similarity [N, N] (GEMM + one scaling pass)."""
    return ops.cosine_sim(x)


class GraphMLPStudent(nn.Module):
    """What the reference's SEMLP is while it trains GraphMLP (:51-75, :101-138 with SEMLP__downgrade_to_MLP): `alphas` ([1e-4, 1e-4], never given
    a gradient) and `part2` = GraphMLP, so that the checkpoint has the reference's keys (alphas, part2.model.0.weight, ...,
    part2.out_proj.bias) and loads from a reference checkpoint and into one.  part2 is built lazily by the first forward_part2, as there."""

    def __init__(self, args, data):
        super().__init__()
        self.args = args
        self.train_mask, self.test_mask = data.train_mask, data.test_mask
        self.train_idx, self.test_idx = data.train_idx, data.test_idx
        if self.args.batch_size > len(self.train_idx):
            print(f'\n\n    Batch size too large...\n Changing batch_size from {self.args.batch_size} to {len(self.train_idx)}!\n\n')
            self.args.batch_size = len(self.train_idx)
        self.part2 = None
        self.alphas = nn.Parameter(torch.tensor([0.0001, 0.0001]), requires_grad=True)
        self.loss_NContrastive = None
        self.on_build = None
        self._idx = (None, None)

    index_on_device = SEMLP.index_on_device

    def forward_part2(self, x, batch_idx=None, edge_index=None):
        if batch_idx is not None:
            x = ops.gather_rows_by_index(x, self.index_on_device(batch_idx, x.device))
        if self.part2 is None:
            self.part2 = GraphMLP(self.args, self.train_mask)
            if self.on_build is not None:
                self.on_build('part2', self.part2)
            if getattr(self, 'optfun', None) is not None:
                self.opt = self.optfun(self.parameters(), lr=self.args.lr, weight_decay=self.args.weight_decay)
        res = self.part2(x, edge_index=edge_index, batch_idx=batch_idx)
        self.loss_NContrastive = res.loss_NContrastive
        return res.emb

    def forward(self, x, edge_index=None):
        return
