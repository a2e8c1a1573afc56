#!/usr/bin/env python3
"""GIST training of the small full-graph GCN (Cora / Citeseer / Pubmed): the command line and the printed lines of
the reference's gcn/train_ist.py -- flags and defaults :311-338, the two shape asserts :62,83, the data-statistics block
:92-101, the per-epoch line :296-298 and the three result lines :304-306 -- over gist_amd.gcn_ist.GISTFullGraphTrainer
(dispatch / step / merge on the HIP kernels, the sub-GCNs' whole-tensor layer norm on the grid-wide kernels).

    python -m gist_amd.scripts.gcn_train_ist --dataset cora-synth --num_subnet 2 --n-epochs 200

`--dataset cora|citeseer|pubmed` need the real files (none offline: an error, never a silent substitute); `cora-synth`
is the seeded Cora-like stand-in of SURVEY.md section 8d.  `--use_random_proj True` densifies the features with a
Gaussian random projection to in_feats // S * S columns (:72-81): the matrix is drawn on the host with numpy as
N(0, 1 / n_components), the distribution sklearn's GaussianRandomProjection documents, and the product runs on the device
(sklearn is not needed).
"""
import argparse
import copy
import warnings

import numpy as np

from gist_amd.scripts.gcn_train import CITATION_SETS, _flag

STRING_FLAGS = ('use_ist', 'split_input', 'split_output', 'self_loop', 'use_layernorm', 'use_random_proj')


def build_parser():
    ap = argparse.ArgumentParser(description='GCN')
    add = ap.add_argument
    add("--dataset", type=str, default="cora")
    add("--data-root", type=str, default=None)
    add("--use_ist", type=str, default="True", help="whether use IST training")
    add("--iter_per_site", type=int, default=5)
    add("--num_subnet", type=int, default=2, help="number of sub networks")
    add("--dropout", type=float, default=0.5, help="dropout probability")
    add("--split_output", type=str, default="False")
    add("--split_input", type=str, default="True")
    add("--gpu", type=int, default=1, help="gpu")
    add("--lr", type=float, default=0.01, help="learning rate")
    add("--n-epochs", type=int, default=200, help="number of training epochs")
    add("--n-hidden", type=int, default=16, help="number of hidden gcn units")
    add("--n-layers", type=int, default=1, help="number of hidden gcn layers")
    add("--weight-decay", type=float, default=5e-4, help="Weight for L2 loss")
    add("--self_loop", type=str, default='True', help="graph self-loop (default=True)")
    add("--use_layernorm", type=str, default='True', help="Whether use layernorm (default=False)")
    add("--use_random_proj", type=str, default='True',
        help="Whether use random projection to densitify (default=False)")
    return ap


def string_flags(args):
    """The reference's string booleans (:42-59): each exactly 'True' or 'False', else an AssertionError."""
    return {name: _flag(args, name) for name in STRING_FLAGS}


def random_projection(features, n_components, device, rs=np.random):
    """features [N, F] @ R [F, n_components], R ~ N(0, 1 / n_components) drawn on the host, the product on the device."""
    import torch
    from gist_amd import autograd
    R = rs.normal(0.0, 1.0 / np.sqrt(n_components), (features.shape[1], n_components)).astype(np.float32)
    x = torch.as_tensor(np.asarray(features, np.float32)).to(device)
    with torch.no_grad():
        return autograd.matmul(x, torch.from_numpy(R).to(device)).cpu().numpy()


def _mean(xs):
    """np.mean, [] -> nan without the warning (the reference prints nan before the fourth epoch)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return float(np.mean(xs))


def main(args, data=None, log=print, init_params=None, partitions=None):
    import torch
    from gist_amd.gcn_ist import GISTFullGraphTrainer
    f = string_flags(args)
    assert (args.n_hidden % args.num_subnet) == 0
    if data is None:
        if args.dataset not in CITATION_SETS:
            raise NotImplementedError('%s is not a valid dataset' % args.dataset)
        from gist_amd.dgl_compat.data import load_data
        data = load_data(args)
    if not f['use_ist']:                                   # :289 (the reference gets there in its first epoch)
        raise NotImplementedError('Should train with IST')
    # --gpu is parsed and, as in the reference (:102), not used: the run is on the current device
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
    if f['use_random_proj']:
        if device is None:
            raise RuntimeError('gist_amd: the random projection runs on the HIP kernels and needs a GPU')
        n_components = int(data.features.shape[-1] / args.num_subnet) * args.num_subnet
        data = copy.copy(data)
        data.features = random_projection(data.features, n_components, device)
    else:
        assert (data.features.shape[-1] % args.num_subnet) == 0.
    t = GISTFullGraphTrainer(data, args.n_hidden, args.n_layers, args.dropout, f['use_layernorm'], args.lr,
                             args.weight_decay, num_subnet=args.num_subnet, iter_per_site=args.iter_per_site,
                             split_input=f['split_input'], split_output=f['split_output'], self_loop=f['self_loop'],
                             device=device, init_params=init_params)
    sizes = t.mask_sizes()
    log("----Data statistics------'\n"
        "      #Edges %d\n      #Classes %d\n      #Train samples %d\n      #Val samples %d\n"
        "      #Test samples %d" % (t.n_edges_raw, t.n_classes, sizes['train'], sizes['val'], sizes['test']))

    def line(epoch, loss):
        dur = _mean(t.step_seconds)
        val, test = t.history[-1]
        log("Epoch {:05d} | Time(s) {:.4f} | Loss {:.4f} | Val Accuracy {:.4f} | Test Accuracy {:.4f} |"
            "ETputs(KTEPS) {:.2f}".format(epoch, dur, loss.item(), val, test, t.n_edges / dur / 1000))

    t.fit(args.n_epochs, partitions=partitions, on_epoch=line)
    final = t.accuracy('test')
    log("Final Test Accuracy: %.4f" % final)
    log("Best Val Accuracy: %.4f" % max(v for v, _ in t.history))
    log("Best Test Accuracy: %.4f" % max(s for _, s in t.history))
    site_losses = [[float(l.item()) for l in row] for row in t.site_losses]
    return dict(model=t.model, losses=[row[-1] for row in site_losses], record=[list(r) for r in t.history],
                final_test=final, n_edges=t.n_edges,
                epoch_time=float(np.mean(t.step_seconds)) if t.step_seconds else None,
                site_losses=site_losses, merged=t.merged)


if __name__ == '__main__':
    main(build_parser().parse_args())
