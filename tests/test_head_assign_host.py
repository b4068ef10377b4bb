"""CPU-side checks of the device assignment solver's entry points (csrc/head_assign.hip): the argument checks that come before any
GPU call, the two pure host functions, the head's ``assign_on`` switch and the tool's resource listing."""
import copy
import ctypes
import json
import os
import pickle
import subprocess
import sys

import pytest

import test_head_train_host as H
from sparsebev_amd import _lib
from sparsebev_amd import head_train as HT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = ctypes.c_void_p(64)          # a non-null pointer that a refused call never dereferences


def call(L, B, Q, Gmax, cost=PTR, offsets=PTR, assign=PTR, status=PTR, workspace=PTR):
    return _lib.load().sbev_head_assign_device(cost, offsets, L, B, Q, Gmax, assign, status, workspace, None)


def test_refusals_come_before_any_gpu_call():
    lib = _lib.load()
    for sizes in ((-1, 1, 4, 2), (1, -1, 4, 2), (1, 1, -4, 2), (1, 1, 4, -2), (1, 1, 0x8000, 2)):
        assert call(*sizes) == -1 and b'sbev_head_assign_device' in lib.sbev_last_error(), sizes
    for name in ('cost', 'offsets', 'assign', 'workspace'):
        assert call(1, 1, 0x7fff, 2, **{name: None}) == -1, name        # Q = 0x7fff: the state lives in the workspace
        msg = lib.sbev_last_error()
        assert b'sbev_head_assign_device' in msg and b'null' in msg, (name, msg)
    # L * B * Q == 0: nothing to do, nothing looked at
    for sizes in ((0, 3, 4, 2), (3, 0, 4, 2), (3, 3, 0, 2)):
        assert call(*sizes, cost=None, offsets=None, assign=None, status=None, workspace=None) == 0, sizes


def test_workspace_and_plan_are_pure_host_functions():
    lib = _lib.load()
    ws, plan = lib.sbev_head_assign_device_workspace, lib.sbev_head_assign_device_plan
    for sizes in ((-1, 1, 4, 2), (1, -1, 4, 2), (1, 1, -4, 2), (1, 1, 4, -2), (1, 1, 0x8000, 2)):
        assert ws(*sizes) == -1, sizes
    assert plan(-1, 2) == -1 and plan(4, -1) == -1 and plan(0x8000, 2) == -1
    assert plan(900, 40) == 0                   # the training shape keeps its state in LDS
    assert plan(0x7fff, 40) == 1 and plan(0x7fff, 0) == 1
    assert plan(36, 5) == 0 and plan(5, 300) == 0 and plan(5, 0x7fff) == 1      # more boxes than queries: the boxes are the columns
    base = (6, 2, 3000, 40)                     # beyond LDS: the workspace holds the state
    assert plan(base[2], base[3]) == 1 and ws(*base) >= 6 * 2 * (29 * 3000 + 13 * 40)
    for k in range(4):
        prev = ws(*base)
        for step in (1, 7, 500):
            grown = list(base)
            grown[k] += step
            assert ws(*grown) >= prev, (k, step)
            prev = ws(*grown)
    prev = 0
    for Q in range(0, 4000, 37):                # across the LDS threshold as well
        assert ws(2, 3, Q, 5) >= prev
        prev = ws(2, 3, Q, 5)
    assert ws(0, 3, 900, 40) == 0 and ws(6, 1, 900, 40) >= 0


def test_assign_on_switch():
    host, dev = H.make_head(), H.make_head(assign_on='device', **H.CONFIG)
    assert host.assign_on == 'host' and H.make_head(assign_on='host').assign_on == 'host' and dev.assign_on == 'device'
    assert host.assign_status is None and dev.assign_status is None
    for bad in ('gpu', 'cuda', None, 1):
        with pytest.raises(ValueError, match='assign_on'):
            H.make_head(assign_on=bad)
    assert len(dev.state_dict()) == 51 and list(dev.state_dict()) == list(host.state_dict())
    dev.load_state_dict(host.state_dict(), strict=True)
    twin = copy.deepcopy(dev)
    assert twin.assign_on == 'device' and twin._assigner is not dev._assigner
    assert pickle.loads(pickle.dumps(dev._assigner))._cost is None
    again = pickle.loads(pickle.dumps(dev))
    assert again.assign_on == 'device' and list(again.state_dict()) == list(dev.state_dict())
    assert dev.eval().assign_on == 'device'


def test_tool_lists_the_kernel_with_zero_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'bench_head_train.py'), '--resources-only'], stdout=subprocess.PIPE,
                         check=True, cwd=ROOT).stdout.decode()
    res = json.loads(out.strip().splitlines()[-1])
    lds, ws = 'head_assign_kernel<true>', 'head_assign_kernel<false>'            # the state in LDS / in the workspace
    assert lds in res and ws in res and 'match_cost_kernel' in res and 'set_loss_kernel' in res
    for name, r in res.items():
        assert r['scratch_bytes_per_lane'] == 0, name
    assert res[ws]['lds_bytes_per_block'] < res[lds]['lds_bytes_per_block'] <= 64 * 1024
