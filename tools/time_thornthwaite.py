"""What Thornthwaite PET from the members' own air temperature costs at BASELINE C3's size (100 000 members x 10 957 days), with
the snow module in the kernel (the three-row forcing table the PET model needs).

Sibling of tools/time_forcing_error.py, same method: device-resident timings with torch events, one warm-up and ``--repeats``
repeats per leg, and a generator's time is (the run with ``forcing_error``) - (the same run handed the kept table explicitly),
so the main launch reads the same numbers in both.  Two generators in one session:
  A. a T_air offset per member, no PET model: the independent generator of the parent commit on three rows;
  B. the same with ``'PET': {'model': 'thornthwaite'}``: generator A writing F = 1.0 into the PET row, then the PET kernel.
B - A is the PET kernel.  ``--pet-scale`` gives every member a PET scale in both, so that the PET kernel also reads F.
Prints one JSON line; ``--md FILE`` also writes the figures as a table.  ``--members`` / ``--years`` shrink the problem.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--years', type=int, default=30, help='whole years from 1981')
    ap.add_argument('--latitude', type=float, default=57.1)
    ap.add_argument('--pet-scale', action='store_true')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()

    import torch
    from simplyp_amd import engine, forcing, marshal, synthetic
    E = args.members
    pr = synthetic.c3_problem(E, end_dt='%d-12-31' % (1980 + args.years), solver=dict(out_slot_order=1))
    pr['forcing'], pr['doy'] = marshal.forcing_arrays(pr['met'], snow=True)
    pr['opts'].snow = 1
    D = pr['forcing'].shape[2]
    eng = engine.get_engine(0)
    rng = np.random.default_rng(1)
    base = {'T_air': {'offset': rng.uniform(-1.0, 4.0, E)}}
    if args.pet_scale:
        base['PET'] = {'scale': rng.uniform(0.9, 1.1, E)}
    with_model = dict(base, PET=dict(base.get('PET', {}), model='thornthwaite', latitude=args.latitude))
    dev = {k: eng.to_device(pr[k]) for k in ('forcing', 'doy', 'member_params', 'reach_params')}
    out = torch.empty((5, D, 1, E), dtype=torch.float64, device=eng.tdev)
    mos = torch.empty((E,), dtype=torch.int32, device=eng.tdev)
    ident = torch.arange(E, dtype=torch.int32, device=eng.tdev)

    def one(f, **kw):
        return eng.run(f, dev['doy'], dev['member_params'], dev['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'], out=out,
                       member_of_slot=mos, **kw)[2]

    def timed(fn):
        fn()                                                    # warm-up
        ms, stats = [], None
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            stats = fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms, stats

    torch.cuda.synchronize(eng.tdev)
    stream = torch.cuda.Stream(eng.tdev)
    legs = {}
    with torch.cuda.stream(stream):
        for name, spec in (('A', base), ('B', with_model)):
            fe = forcing.resolve(spec, pr['met'].index, E, True, seed=1)
            ms1, st1 = timed(lambda: one(dev['forcing'], forcing_error=fe))
            table = one(dev['forcing'], forcing_error=fe, keep_forcing_table=True)['forcing_table']
            ms2, st2 = timed(lambda: one(table, forcing_of_member=ident))
            del table
            legs[name] = dict(with_forcing_error_ms=ms1, explicit_table_ms=ms2, kernel_ms=[st1['kernel_ms'], st2['kernel_ms']],
                              generator_ms=float(np.median(ms1) - np.median(ms2)))
    row_bytes = E * D * 8
    pet_ms = legs['B']['generator_ms'] - legs['A']['generator_ms']
    pet_bytes = row_bytes * (3 if args.pet_scale else 2)          # T_air read, PET written; F read with a scale
    res = dict(members=E, days=D, years=args.years, pet_scale=bool(args.pet_scale), table_bytes=3 * row_bytes, legs=legs,
               pet_kernel_ms=pet_ms, pet_kernel_bytes=pet_bytes, pet_kernel_gbs=pet_bytes / pet_ms / 1e6 if pet_ms > 0 else None,
               generator_a_write_gbs=3 * row_bytes / legs['A']['generator_ms'] / 1e6 if legs['A']['generator_ms'] > 0 else None)
    print(json.dumps(res))
    if args.md:
        med = lambda x: float(np.median(x))
        with open(args.md, 'w') as fh:
            fh.write("| generator (%d members x %d days, 3 rows%s) | (1) with forcing_error, median ms (repeats) | (2) kept table given, median ms (repeats) "
                     "| generator ms | main launch ms (1) |\n|---|---|---|---|---|\n" % (E, D, ', PET scale' if args.pet_scale else ''))
            for name, label in (('A', 'A. T_air offset, no PET model'), ('B', 'B. the same with Thornthwaite PET')):
                g = legs[name]
                fh.write("| %s | %.1f (%s) | %.1f (%s) | %.1f | %.1f |\n"
                         % (label, med(g['with_forcing_error_ms']), ', '.join('%.1f' % x for x in g['with_forcing_error_ms']),
                            med(g['explicit_table_ms']), ', '.join('%.1f' % x for x in g['explicit_table_ms']), g['generator_ms'], g['kernel_ms'][0]))
            fh.write("\nPET kernel (B - A): %.1f ms for %.2f GB = %s GB/s.  Generator A: %.2f GB of table writes = %s GB/s.\n"
                     % (pet_ms, pet_bytes / 1e9, 'n/a' if pet_ms <= 0 else '%.0f' % res['pet_kernel_gbs'], 3 * row_bytes / 1e9,
                        'n/a' if res['generator_a_write_gbs'] is None else '%.0f' % res['generator_a_write_gbs']))


if __name__ == '__main__':
    main()
