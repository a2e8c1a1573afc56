"""TEST INFRASTRUCTURE (not product): one rank of GIST for the GraphSAGE family in its own process on the box's one GPU,
the collective host-staged over gloo (tests/host_staged_comm.py); everything else is the product path (the grouped
mover, the fused step, the script).

    python tests/graphsage_ist_worker.py step   RANK S PORT OUT.json L P_DROP USE_PP
        tests/graphsage_ist_step_check.run_and_replay for this rank -> {errors, events, base (sha256)}
    python tests/graphsage_ist_worker.py script RANK S PORT OUT.json HOST_PATH WORKDIR
        the script's main twice, --eval-path layers (result lines) then rows (--save_results, under WORKDIR)
        -> {errors, lines, pickle and, per eval path, val_*, test_*, events_*, steps_*, base_* (sha256 of the replica)}"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCRIPT_ARGV = ['--dataset', 'toy', '--n-epochs', '16', '--batch-size', '4', '--n-hidden', '32', '--n-layers', '2',
               '--iter_per_site', '5', '--weight-decay', '0', '--rnd-seed', '0', '--dropout', '0.1', '--lr', '0.01',
               '--dist-backend', 'gloo', '--use_layernorm', 'True']


def labelled_toy():
    """datasets.toy() with labels its neighbourhoods determine (tests/test_ist_gat_gpu.py builds the same)."""
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
    from tests.graphsage_ist_step_check import run_and_replay
    from tests.host_staged_comm import HostStagedComm
    L, p_drop, use_pp = int(argv[0]), float(argv[1]), argv[2] == '1'
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=S)
    errs, events, facts = run_and_replay(S, L, p_drop, use_pp, dev, [rank], lambda r: HostStagedComm())
    dist.barrier()
    dist.destroy_process_group()
    return dict(errors=errs, events=events, base=hashlib.sha256(facts['base'].numpy().tobytes()).hexdigest())


def run_script(rank, S, port, argv):
    import pickle
    from gist_amd.scripts import cluster_gcn_ist_distrib_graphsage as cli
    from tests.host_staged_comm import HostStagedComm
    host_path, workdir = argv[0], argv[1]
    os.chdir(workdir)
    out = dict(errors=[])
    for n, eval_path in enumerate(('layers', 'rows')):
        lines = []
        argv_n = SCRIPT_ARGV + ['--num_subnet', str(S), '--rank', str(rank), '--host-path', host_path, '--eval-path',
                                eval_path, '--dist-url', 'tcp://127.0.0.1:%d' % (port + n)]
        if eval_path == 'rows':
            argv_n += ['--save_results', '--exp_name', 'graphsage_%s' % host_path]
        res = cli.main(cli.build_parser().parse_args(argv_n), dataset=labelled_toy(),
                       log=lambda *a, **k: lines.append(' '.join(map(str, a))), comm=HostStagedComm())
        out['val_' + eval_path], out['test_' + eval_path] = res['val_accs'], res['test_accs']
        # what the ranks must agree on: the schedule each one ran, and its base replica after the last sync, bit for bit
        out['events_' + eval_path] = res['events']
        out['base_' + eval_path] = hashlib.sha256(res['model'].base.params.cpu().numpy().tobytes()).hexdigest()
        out['steps_' + eval_path] = len(res['losses'][0])
        if eval_path == 'layers':
            out['lines'] = lines[-5:] if rank == 0 else []
        elif rank == 0:
            out['saw_lines'] = any(l.startswith('Training Time') for l in lines)
            got = pickle.load(open(res['results_path'], 'rb'))
            out['pickle'] = dict(keys=sorted(got), val_accs=got['val_accs'], path=os.path.abspath(res['results_path']))
    return out


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
