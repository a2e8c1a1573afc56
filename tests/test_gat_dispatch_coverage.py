"""CPU: the width cases of test_gat_kernels_gpu.py reach every (VEC, LPG) instantiation of the GAT walkers with one
column pass and, where F allows, with several, through a mirror of gat.hip's gat_vec4 / gat_lpg dispatch."""
from tests.test_gat_kernels_gpu import case_dispatch, walker_dispatch


def _reachable(max_f=4096):
    """Every (VEC, LPG, 1 or 2 = several passes) some width reaches: VEC = 4 needs F % 4 == 0 (and alignment)."""
    out = set()
    for f in range(1, max_f + 1):
        for aligned in (False, True):
            vec, lpg, passes = walker_dispatch(f, aligned)
            out.add((vec, lpg, min(passes, 2)))
    return out


def test_gat_cases_cover_every_walker_instantiation():
    reach = _reachable()
    assert {(v, l) for v, l, _ in reach} == {(v, l) for v in (1, 4) for l in (8, 16, 32, 64)}
    covered = {}
    for (vec, lpg, passes), widths in case_dispatch().items():
        covered.setdefault((vec, lpg, min(passes, 2)), []).extend(widths)
    table = '\n'.join('  VEC=%d LPG=%-2d %s: F %s' % (v, l, 'one pass' if p == 1 else 'several passes',
                                                    covered.get((v, l, p), 'NOT COVERED'))
                      for v, l, p in sorted(reach))
    print('\nGAT walker instantiations reached by the kernel tests:\n' + table)
    assert set(covered) == reach, 'uncovered walker dispatch:\n' + table
