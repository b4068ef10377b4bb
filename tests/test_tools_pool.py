"""tools/bench_pool.py: its argument parsing and the figures of its JSON line, without a GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


def test_bench_pool_arguments_and_summary():
    import bench_pool as BP
    a = BP.parse_args([])
    assert (a.config, a.steps, a.warmup, a.rounds, a.ring_slots, a.pool_slots) == ('c2', 50, 40, 3, None, 16)
    assert BP.CONFIGS['c2'] == ('r50_704x256', 900, 8)                  # the flagship streaming shape: B = 1, T = 8
    a = BP.parse_args(['--config', 'small', '--steps', '5', '--warmup', '0', '--rounds', '2', '--pool-slots', '12', '--ring-slots', '9'])
    assert (a.config, a.steps, a.warmup, a.rounds, a.ring_slots, a.pool_slots) == ('small', 5, 0, 2, 9, 12)
    for bad in (['--steps', '0'], ['--rounds', '0'], ['--warmup', '-1'], ['--pool-slots', '17'], ['--pool-slots', '0'], ['--config', 'c9']):
        with pytest.raises(SystemExit):
            BP.parse_args(bad)
    s = BP.summarise([2.0, 1.0, 3.0], [2.2, 4.0, 1.1])
    assert s['ring_median_ms'] == 2.0 and s['pool_median_ms'] == 2.2 and s['pool_over_ring'] == 1.1
    assert s['ring_ms_per_step'] == [2.0, 1.0, 3.0] and s['pool_ms_per_step'] == [2.2, 4.0, 1.1]
