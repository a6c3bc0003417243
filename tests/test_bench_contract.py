"""bench.py's JSON contract (static checks; the numbers themselves need the GPU)."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_has_contract_keys():
    src = open(os.path.join(ROOT, 'bench.py')).read()
    ast.parse(src)
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"',
                '"higher_is_better"', '"scaling"', '"vs_baseline"', '"dtype"', '"data"', '"config"', '"workload"',
                '"roofline"', '"bound"', '"achieved"', '"peak"', '"frac"', '"traffic"', '"cpu_baseline"', '"cores"',
                '"kind"', '"sample"', '"members_total"', '"rccl_ranks"', '"per_rank"', '"kernel_ms"', "'value_weak'", "'secondary'"):
        assert key in src, key
    assert "'--gpus'" in src and "'--steps'" in src and "'--warmup'" in src


def test_default_scaling_is_baseline_c3_as_stated():
    """BASELINE C3 = ONE 100 000-member ensemble sharded over 1 -> 8 GPUs: `python bench.py --gpus N` must time that (strong),
    and never quietly something else; the other configs keep per-GPU sizes (weak)."""
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    a = bench.parse_args(['--gpus', '8'])
    assert a.scaling is None and a.config == 'c3' and bench.CONFIGS['c3']['scaling'] == 'strong' and bench.CONFIGS['c3']['members'] == 100000
    assert all(bench.CONFIGS[c]['scaling'] == 'weak' for c in ('c2', 'c4', 'c5'))
    assert bench.parse_args(['--scaling', 'weak']).scaling == 'weak'
    src = open(os.path.join(ROOT, 'bench.py')).read()
    assert 'raise SystemExit(3)' in src and 'table left in HBM on every rank' not in src       # no silent fallback of what `value` means


def test_steps_must_be_positive():
    import importlib
    import sys
    import pytest
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    assert bench.parse_args(['--steps', '5']).steps == 5
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_full_is_off_by_default():
    """A plain run times the headline alone; everything else the bench measures waits for --full."""
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    assert bench.parse_args([]).full is False
    assert bench.parse_args(['--full', '--no-secondary']).full is True


def test_dump_outputs_in_member_order_and_within_budget(tmp_path):
    """--dump-outputs: the table's slot order is resolved to member order, a table larger than the budget is cut to a seeded
    member sample (the same one on every call), everything is float64 and the files stay under 64 MB in all."""
    import importlib
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    n_cols, rows, E = 5, 10957, 300                  # 300 members of C3's table: 131 MB, more than the dump may hold
    rng = np.random.default_rng(0)
    mos = rng.permutation(E)                         # member_of_slot
    table = np.empty((n_cols, rows, 1, E))
    table[...] = mos.astype(np.float64)              # every value of a slot names its member
    table[:, :, 0, :] += np.arange(rows, dtype=np.float64)[None, :, None] * 1e-6
    summ = torch.arange(n_cols * E, dtype=torch.float64).reshape(n_cols, 1, E)
    status = torch.zeros(E, dtype=torch.int32)
    written = [bench.dump_outputs(str(tmp_path / d), table, torch.as_tensor(mos), summ, status) for d in ('a', 'b')]
    assert written[0] == written[1]
    total = 0
    for name in written[0]:
        a, b = (np.load(str(tmp_path / d / (name + '.npy'))) for d in ('a', 'b'))
        assert a.dtype == np.float64 and np.array_equal(a, b)
        total += (tmp_path / 'a' / (name + '.npy')).stat().st_size
    assert total <= 64 << 20
    members = np.load(str(tmp_path / 'a' / 'table_members.npy')).astype(np.int64)
    got = np.load(str(tmp_path / 'a' / 'table.npy'))
    assert 0 < len(members) < E and got.shape == (n_cols, rows, 1, len(members))
    assert np.array_equal(np.floor(got[0, 0, 0]), members)
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'summaries.npy')), summ.numpy())
    assert 'summaries_members' not in written[0]
