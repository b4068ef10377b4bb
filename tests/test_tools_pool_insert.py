"""tools/bench_pool.py's third leg (the pool fed through FramePool.step): the additive summary fields, from made-up per-round times,
without a GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


def test_bench_pool_step_leg_summary():
    import bench_pool as BP
    two = BP.summarise([2.0, 1.0, 3.0], [2.2, 4.0, 1.1])
    three = BP.summarise([2.0, 1.0, 3.0], [2.2, 4.0, 1.1], [1.1, 3.3, 1.65])
    assert {k: three[k] for k in two} == two                                # additive: the two-leg figures are what they were
    assert sorted(set(three) - set(two)) == ['pool_step_median_ms', 'pool_step_ms_per_step', 'pool_step_over_pool']
    assert three['pool_step_ms_per_step'] == [1.1, 3.3, 1.65] and three['pool_step_median_ms'] == 1.65
    assert three['pool_step_over_pool'] == 0.75                             # against the put leg's median of the same run (2.2), not the ring's
    one = BP.summarise([5.0], [4.0], [3.0])
    assert (one['pool_step_median_ms'], one['pool_step_over_pool'], one['pool_over_ring']) == (3.0, 0.75, 0.8)
    assert 'pool_step_median_ms' not in BP.summarise([5.0], [4.0])

