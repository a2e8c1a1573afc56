"""CPU: the cases of test_spmm_kernels_gpu.py reach every aggregation kernel instantiation, through that module's mirror
of the host dispatch (spmm.hip spmm_choose / spmm_generic / launch_spmm / spmm_prepared_takes / l2_split_for,
spmm_dense32.hip spmm_dense32_takes and its row-tile choice); and the mirror agrees with the library's
own answers (gist_spmm_drop_takes, gist_spmm_prepared_useful) over a grid of widths, pitches, pointer alignments, row
blocks and every spmm_kernel tuning value, so a change to the C++ dispatch the mirror misses fails here."""
import itertools

from tests.test_spmm_kernels_gpu import (CASES, case_coverage, every_instantiation, case_instantiations,
                                         spmm_drop_takes, spmm_prepared_takes)


def test_spmm_cases_cover_every_instantiation():
    cov = case_coverage()
    want = every_instantiation()
    table = '\n'.join('  %-42s %s' % (k, ', '.join(sorted(set(cov[k]))) if k in cov else 'NOT COVERED')
                      for k in sorted(want | set(cov)))
    print('\nSpMM kernel instantiations reached by the kernel tests:\n' + table)
    assert set(cov) == want, 'uncovered or unknown instantiation:\n' + table
    # the LDS kernel under every forced row split, and the automatic one
    splits = {inst[3] for c in CASES for inst in case_instantiations(c) if inst[0] == 'lds2' and not inst[2]}
    assert {1, 2, 3, 16} <= splits, splits


def test_spmm_dispatch_mirror_matches_library():
    from gist_amd import hip, _lib
    L = _lib.load()
    base = 1 << 20                      # pointers are only tested for alignment on these host entry points
    prev = hip.tuning('spmm_kernel')
    try:
        for knob in (0, 1, 2, 3):
            hip.tuning('spmm_kernel', knob)
            for d, pad, ax, ay in itertools.product(
                    (1, 2, 16, 100, 127, 128, 130, 256, 258, 602, 1024, 1534, 1536, 1540, 2048, 4096),
                    (0, 1, 2, 4), (4, 8, 16), (4, 8, 16)):
                ldx, ldy = d + pad, d + (pad * 3) % 5
                xp, yp = base + ax % 16, base + 256 + ay % 16     # (16: 16-byte aligned; 4 / 8: only that)
                for rb in (False, True):
                    for mode in (1, 2):
                        got = bool(L.gist_spmm_drop_takes(mode, d, ldx, ldy, xp, yp, int(rb)))
                        want = bool(spmm_drop_takes(mode, d, ldx, ldy, ax, ay, rb, knob))
                        assert got == want, ('drop_takes', knob, mode, d, ldx, ldy, ax, ay, rb)
                got = bool(L.gist_spmm_prepared_useful(d, ldx, ldy, xp, yp))
                want = spmm_prepared_takes(d, ldx, ldy, ax, ay, knob)
                assert got == want, ('prepared_useful', knob, d, ldx, ldy, ax, ay)
    finally:
        hip.tuning('spmm_kernel', prev)
