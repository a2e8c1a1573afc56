"""GIST training of the small full-graph GCN on one GPU: the loop of the reference's `gcn/train_ist.py` (the script
behind the paper's Cora / Citeseer / Pubmed table), which simulates `num_subnet` sub-GCNs in one process.

Every `iter_per_site` epochs the base `gcn.GCN` is cut into S narrower `gcn.GCN`s along random index partitions
(dispatch, :146-207), every sub-GCN takes one full-graph Adam step per epoch (:213-225), and the sub-GCNs are written back
into the base (merge, :237-286), which is what gets scored (:294-299).

`P[i]` partitions layer i's input rows = layer i-1's output columns.  With `has(i)` = "P[i] is a partition, not None",
every tensor moves by one rule (`tensor_plan`):

  W_k    rows P[k][s], columns P[k+1][s]   (k < L; None = all)       W_L  rows P[L][s], all columns
  b_k    entries P[k+1][s]                 (k < L)                   b_L  copied whole
  merge  a tensor gathered through a list is scattered back through the same lists; a tensor gathered with NO list at
         all is the mean over the sites, in site order; b_L is never written back.

The eight branches of :243-285 are this rule; the last clause is the reference's: no branch names
`layers.{n_layers}.bias`, so the base keeps its INITIAL output bias for the whole run while every site trains a copy of it.
The moves are `gist_block_gather_f32` / `gist_block_scatter_f32` / `gist_mean_rows_f32`; the partitions are permutations,
not contiguous blocks, which those kernels take as index lists.
"""
import torch

from . import hip
from .gcn import GCN, FullGraphSetup


def draw_partitions(in_feats, n_hidden, n_layers, num_subnet, split_input, split_output):
    """The index partitions of one dispatch (train_ist.py:150-166), drawn from torch's global CPU generator in the
    reference's order: P[0] = chunks of randperm(in_feats) or None, P[1..n_layers-1] = chunks of randperm(n_hidden),
    P[n_layers] = chunks of randperm(n_hidden) with split_output, else None."""
    P = [torch.chunk(torch.randperm(in_feats), num_subnet) if split_input else None]
    for _ in range(1, n_layers):
        P.append(torch.chunk(torch.randperm(n_hidden), num_subnet))
    P.append(torch.chunk(torch.randperm(n_hidden), num_subnet) if split_output else None)
    return P


def tensor_plan(n_layers, split_input, split_output):
    """[(state-dict name, rows, cols, merge)] of the 2 * (n_layers + 1) tensors: rows / cols = which P[i] indexes that
    axis at dispatch (None = the whole axis; a bias has cols only), merge = 'scatter' (back through the same lists),
    'mean' (over the sites) or 'keep' (never written back: the output bias)."""
    has = [bool(split_input)] + [True] * (n_layers - 1) + [bool(split_output)]
    plan = []
    for k in range(n_layers + 1):
        rows = k if has[k] else None
        cols = k + 1 if k < n_layers and has[k + 1] else None
        plan.append(('layers.%d.weight' % k, rows, cols, 'mean' if rows is None and cols is None else 'scatter'))
        if k < n_layers:
            plan.append(('layers.%d.bias' % k, None, cols, 'mean' if cols is None else 'scatter'))
        else:
            plan.append(('layers.%d.bias' % k, None, None, 'keep'))
    return plan


def site_lr(lr, epoch, n_epochs):
    """The learning rate a site's optimiser is built with at a dispatch in `epoch` (:193-198)."""
    if epoch >= int(n_epochs * 0.5):
        lr /= 10
    if epoch >= int(n_epochs * 0.75):
        lr /= 10
    return lr


class GISTFullGraphTrainer(FullGraphSetup):
    """`gcn/train_ist.py`'s loop body over the HIP kernels.  Data, graph and the base model are set up exactly as in
    gcn.FullGraphTrainer (the same code, gcn.FullGraphSetup).  The sub-GCNs run their whole-tensor layer norm on the
    grid-wide kernels (`whole_norm='grid'`).

    Two departures from the letter of the reference, neither visible in the numbers: the reference builds S fresh
    sub-models at every dispatch and overwrites all of their initial values at once (:171-201); this trainer builds the S
    sub-models ONCE and refills them.  And the site's input columns X[:, P[0][s]] are gathered once per dispatch, not at
    every step (:216-217).  Each dispatch gives each site a fresh Adam (zero moments) at `site_lr`.

    One quirk is reproduced: the base's output bias b_L is dispatched but never merged (see the module docstring)."""

    def __init__(self, data, n_hidden, n_layers, dropout, use_layernorm, lr, weight_decay, num_subnet=2,
                 iter_per_site=5, split_input=True, split_output=False, self_loop=True, device=None, activation=None,
                 init_params=None, whole_norm='grid'):
        from .nn import CrossEntropyLoss
        if n_hidden % num_subnet:
            raise ValueError('gist_amd: n_hidden %d is not a multiple of num_subnet %d' % (n_hidden, num_subnet))
        self._setup(data, n_hidden, n_layers, dropout, use_layernorm, self_loop, device, activation, init_params)
        self.in_feats = self.x.shape[1]
        if split_input and self.in_feats % num_subnet:
            raise ValueError('gist_amd: %d input features are not a multiple of num_subnet %d'
                             % (self.in_feats, num_subnet))
        self.n_hidden, self.n_layers, self.S, self.iter_per_site = n_hidden, n_layers, num_subnet, iter_per_site
        self.split_input, self.split_output = bool(split_input), bool(split_output)
        self.lr, self.weight_decay = lr, weight_decay
        self.plan = tensor_plan(n_layers, split_input, split_output)
        self.sub_models = [GCN(self.g, self.in_feats, n_hidden, self.n_classes, n_layers, self.activation, dropout,
                               use_layernorm, self.split_input, self.split_output, num_subnet,
                               whole_norm=whole_norm).to(self.device) for _ in range(num_subnet)]
        self.criterion = CrossEntropyLoss()
        self.optimizers = [None] * num_subnet
        self.site_x = [self.x] * num_subnet
        self.P = self.idx = None                     # the partitions of the last dispatch and their device index lists
        self._labels32 = self.y.to(torch.int32).contiguous()
        self._masks8 = {k: m.to(torch.uint8).contiguous() for k, m in self.masks.items()}
        self._correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._stage = {}
        self.site_losses, self.history, self.step_seconds, self.merged = [], [], [], []

    # -- index lists ------------------------------------------------------------------------------------------
    def _lists(self, P):
        """P (CPU int64 chunks or None per level) -> int32 device index lists, checked against the sub-model widths."""
        widths = [self.in_feats // self.S] + [self.n_hidden // self.S] * self.n_layers
        ranges = [self.in_feats] + [self.n_hidden] * self.n_layers
        has = [self.split_input] + [True] * (self.n_layers - 1) + [self.split_output]
        if len(P) != self.n_layers + 1:
            raise ValueError('gist_amd: a partition list needs n_layers + 1 = %d levels' % (self.n_layers + 1))
        out = []
        for i, level in enumerate(P):
            if (level is not None) != has[i]:
                raise ValueError('gist_amd: partition level %d does not match the split flags' % i)
            if level is None:
                out.append(None)
                continue
            parts = [torch.as_tensor(p).to(torch.int64).reshape(-1) for p in level]
            if len(parts) != self.S or any(p.numel() != widths[i] for p in parts):
                raise ValueError('gist_amd: partition level %d needs %d lists of %d indices' % (i, self.S, widths[i]))
            if torch.cat(parts).sort().values.tolist() != list(range(ranges[i])):
                raise ValueError('gist_amd: partition level %d is not a partition of range(%d)' % (i, ranges[i]))
            out.append([p.to(torch.int32).to(self.device) for p in parts])
        return out

    @staticmethod
    def _pick(idx, level, s):
        return None if level is None else idx[level][s]

    @staticmethod
    def _as2d(t):
        return t if t.dim() == 2 else t.view(1, -1)

    # -- the three phases -------------------------------------------------------------------------------------
    @torch.no_grad()
    def dispatch(self, epoch, n_epochs, P=None):
        """:146-207.  P: the partitions to use (teacher-forced); None draws them."""
        from .optim import Adam
        if P is None:
            P = draw_partitions(self.in_feats, self.n_hidden, self.n_layers, self.S, self.split_input,
                                self.split_output)
        self.P, self.idx = P, self._lists(P)
        base = dict(self.model.named_parameters())
        lr = site_lr(self.lr, epoch, n_epochs)
        for s, sub in enumerate(self.sub_models):
            dst = dict(sub.named_parameters())
            for name, rows, cols, _ in self.plan:
                hip.block_gather(self._as2d(base[name].data), self._pick(self.idx, rows, s),
                                 self._pick(self.idx, cols, s), self._as2d(dst[name].data))
            if self.split_input:
                xs = torch.empty(self.x.shape[0], self.in_feats // self.S, dtype=torch.float32, device=self.device)
                self.site_x[s] = hip.block_gather(self.x, None, self.idx[0][s], xs)
            self.optimizers[s] = Adam(sub.parameters(), lr=lr, weight_decay=self.weight_decay)

    def step_site(self, s):
        """:213-225: one full-graph step of site s (the statements of FullGraphTrainer.step on its sub-model)."""
        sub, opt = self.sub_models[s], self.optimizers[s]
        sub.train()
        opt.zero_grad()
        m = self.masks['train']
        loss = self.criterion(sub(self.site_x[s])[m], self.y[m])
        loss.backward()
        opt.step()
        return loss.detach()

    @torch.no_grad()
    def merge(self):
        """:237-286 by the one rule of the module docstring."""
        base = dict(self.model.named_parameters())
        subs = [dict(sub.named_parameters()) for sub in self.sub_models]
        for name, rows, cols, how in self.plan:
            if how == 'keep':
                continue
            if how == 'scatter':
                for s in range(self.S):
                    hip.block_scatter(self._as2d(subs[s][name].data), self._pick(self.idx, rows, s),
                                      self._pick(self.idx, cols, s), self._as2d(base[name].data))
                continue
            n = base[name].numel()
            stage = self._stage.get(name)
            if stage is None:
                stage = self._stage[name] = torch.empty(self.S, n, dtype=torch.float32, device=self.device)
            for s in range(self.S):
                stage[s].copy_(subs[s][name].data.reshape(-1))
            hip.mean_rows(stage.view(-1), n, self.S, n, base[name].data.view(-1))

    @torch.no_grad()
    def evaluate(self):
        """:294-299: (val, test) accuracy of the BASE model on the full features, eval mode."""
        self.model.eval()
        logits = self.model(self.x).contiguous()
        acc = []
        for which in ('val', 'test'):
            self._correct.zero_()
            hip.argmax_correct(logits, self._labels32, self._masks8[which], self._correct)
            acc.append(float(self._correct.item()) / float(self.masks[which].sum().item()))
        return tuple(acc)

    def accuracy(self, which):
        return self.evaluate()[('val', 'test').index(which)]

    def snapshot(self):
        """The base parameters as [(W, b)] host arrays."""
        return [(conv.weight.detach().cpu().numpy().copy(), conv.bias.detach().cpu().numpy().copy())
                for conv in self.model.layers]

    def fit(self, n_epochs, partitions=None, untimed=3, on_epoch=None):
        """The epochs of :140-299.  partitions: a list of P lists consumed one per dispatch (None: drawn)."""
        import time
        partitions = list(partitions) if partitions is not None else None
        for epoch in range(n_epochs):
            timed = epoch >= untimed
            if timed:
                torch.cuda.synchronize(self.device)
                t0 = time.time()
            if epoch % self.iter_per_site == 0:
                self.dispatch(epoch, n_epochs, partitions.pop(0) if partitions else None)
            losses = [self.step_site(s) for s in range(self.S)]
            merging = (epoch + 1) % self.iter_per_site == 0 or epoch == n_epochs - 1
            if merging:
                self.merge()
            if timed:
                torch.cuda.synchronize(self.device)
                self.step_seconds.append(time.time() - t0)
            if merging:
                self.merged.append(self.snapshot())
            self.site_losses.append(losses)
            self.history.append(self.evaluate())
            if on_epoch is not None:
                on_epoch(epoch, losses[-1])
        return self
