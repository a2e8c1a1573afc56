"""TEST INFRASTRUCTURE (not product): one rank of GIST for the BaselineGCN family in its own process on the box's one GPU,
the collective host-staged over gloo (tests/host_staged_comm.py); everything else is the product path (the grouped
mover, the fused step, the script).

    python tests/baseline_gcn_ist_worker.py step   RANK S PORT OUT.json L P_DROP USE_LAYERNORM H
        tests/baseline_gcn_ist_step_check.run_and_replay for this rank -> {errors, events, base (sha256)}
    python tests/baseline_gcn_ist_worker.py script RANK S PORT OUT.json HOST_PATH N_EPOCHS LR
        the script's main -> {errors, lines, val, test, events, steps, base (sha256 of the replica), views}"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCRIPT_ARGV = ['--dataset', 'toy', '--batch-size', '4', '--n-hidden', '32', '--n-layers', '2', '--iter_per_site', '5',
               '--weight-decay', '0', '--rnd-seed', '0', '--dropout', '0.1', '--dist-backend', 'gloo',
               '--use_layernorm', 'True']


def labelled_toy():
    """datasets.toy() with labels its neighbourhoods determine, as tests/test_baseline_gcn_cli_gpu.py relabels it."""
    import torch
    from gist_amd import datasets
    ds = datasets.toy()
    g = ds.g
    n = g.number_of_nodes()
    rp = g.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    agg = torch.zeros(n, ds.num_classes).index_add_(0, rows, g.ndata['feat'][g.col.long(), :ds.num_classes])
    g.ndata['label'] = agg.argmax(1).to(g.ndata['label'].dtype)
    return ds


def run_step(rank, S, port, argv):
    import torch
    import torch.distributed as dist
    from tests.baseline_gcn_ist_step_check import run_and_replay
    from tests.host_staged_comm import HostStagedComm
    L, p_drop, use_layernorm, H = int(argv[0]), float(argv[1]), argv[2] == '1', int(argv[3])
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
    errs, events, facts = run_and_replay(S, H, L, p_drop, use_layernorm, dev, [rank], lambda r: HostStagedComm())
    dist.barrier()
    dist.destroy_process_group()
    return dict(errors=errs, events=events, base=hashlib.sha256(facts['base'].numpy().tobytes()).hexdigest(),
                resets=facts['resets'])


def run_script(rank, S, port, argv):
    from gist_amd.scripts import cluster_gcn_ist_distrib_baseline as cli
    from tests.host_staged_comm import HostStagedComm
    host_path, n_epochs, lr = argv[0], argv[1], argv[2]
    lines = []
    args = cli.build_parser().parse_args(SCRIPT_ARGV + ['--num_subnet', str(S), '--rank', str(rank), '--host-path',
                                                        host_path, '--n-epochs', n_epochs, '--lr', lr, '--dist-url',
                                                        'tcp://127.0.0.1:%d' % port])
    res = cli.main(args, dataset=labelled_toy(), log=lambda *a, **k: lines.append(' '.join(map(str, a))),
                   comm=HostStagedComm())
    model = res['model']
    # after training the sub-model's Parameters are still the arena's views, and the model is the wrapper's family
    views = ([p.data_ptr() for p in model.sub_model.parameters()] == [v.data_ptr() for v in model.sub.param_views()]
             and type(model).__name__ == 'DistributedBaselineGCNWrapper' and bool(model.sub_model.use_layernorm))
    return dict(errors=[], lines=lines[-5:] if rank == 0 else [], val=res['val_accs'], test=res['test_accs'],
                events=res['events'], steps=len(res['losses'][0]), views=views,
                base=hashlib.sha256(model.base.params.cpu().numpy().tobytes()).hexdigest())


def main():
    mode, rank, S, port, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    try:
        result = (run_step if mode == 'step' else run_script)(rank, S, port, sys.argv[6:])
    except Exception as e:
        import traceback
        result = dict(errors=['EXC ' + repr(e) + traceback.format_exc()])
    with open(out, 'w') as f:
        json.dump(result, f)


if __name__ == '__main__':
    main()
