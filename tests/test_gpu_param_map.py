"""GPU: the parameter map's kernel alone (mpcasm_params_map) against its host restatement
(tests/param_map_restatement.py), the whole buffer compared bit for bit as int64: elements no record names and
rows past the launch carry NaNs with payloads of their own and must keep them."""
import numpy as np
import pytest

import param_map_restatement as pm
from mpcasm import capi, problems

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (7, 3, 2, 3), (82, 18, 4, 257), (83, 300, 9, 4099)]
EXTRA_ROWS = 3


@pytest.fixture
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def nan_payloads(rows, cols):
    """Quiet NaNs, every element with a payload of its own."""
    bits = np.int64(0x7FF8000000000000) | (1 + np.arange(rows * cols, dtype=np.int64))
    return bits.view(np.float64).reshape(rows, cols).copy()


def records(rng, n_params, nrecs, ncmd):
    """``nrecs`` records: as many valid ones as the row has room for with one element left alone (distinct dst,
    every mix of SIGNED and CONST), the rest out of range in one way or another, in random order."""
    valid = min(nrecs, max(n_params - 1, 1))
    dst = rng.permutation(n_params)[:valid]
    recs = np.zeros((nrecs, 4), dtype=np.int32)
    recs[:valid, 0] = dst
    recs[:valid, 1] = rng.integers(0, ncmd, valid)
    recs[:valid, 2] = np.arange(valid) % 4                      # none, SIGNED, CONST, both
    for r in range(valid, nrecs):
        how = (r - valid) % 4
        recs[r] = [(-1, 0, 0, 0), (n_params, 0, 0, 0), (int(rng.integers(0, n_params)), ncmd, 0, 0),
                   (int(rng.integers(0, n_params)), 0, 4 + (r % 4), 0)][how]
    coef = rng.normal(0, 2.0, (nrecs, 2))
    order = rng.permutation(nrecs)
    return recs[order], coef[order]


def launch(torch, params, recs, coef, cmd, stride, ncmd, index, sign, batch):
    from mpcasm.engine import _stream_handle
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = capi.load().mpcasm_params_map(params.data_ptr(), params.shape[1], ptr(recs), ptr(coef), recs.shape[0],
                                       cmd.data_ptr(), stride, ncmd, ptr(index), ptr(sign), batch,
                                       _stream_handle(torch, None))
    assert rc == capi.OK, (rc, capi.load().mpcasm_last_hip())


def same_bits(dev, ref):
    got = dev.cpu().numpy().view(np.int64)
    want = np.ascontiguousarray(ref).view(np.int64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())


# ---- 6. shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_shape_and_way_of_reading_the_commands(torch_gpu, shape):
    torch = torch_gpu
    n_params, nrecs, ncmd, batch = shape
    rng = np.random.default_rng(sum(shape))
    recs, coef = records(rng, n_params, nrecs, ncmd)
    sign = rng.choice([-1.0, 1.0], batch)
    stride = ncmd + 1                                     # (a table wider than the columns the map may name)
    table = rng.normal(0, 1.0, (2 * batch + 1, stride))
    d_recs, d_coef = torch.as_tensor(recs, device="cuda"), torch.as_tensor(coef, device="cuda")
    d_sign, d_table = torch.as_tensor(sign, device="cuda"), torch.as_tensor(table, device="cuda")
    cases = {"in order": None, "permuted": rng.permutation(batch).astype(np.int32),
             "picked from a table": rng.integers(0, 2 * batch + 1, batch).astype(np.int32)}
    start = nan_payloads(batch + EXTRA_ROWS, n_params)
    for name, index in cases.items():
        params = torch.as_tensor(start, device="cuda")
        d_index = None if index is None else torch.as_tensor(index, device="cuda")
        launch(torch, params, d_recs, d_coef, d_table, stride, ncmd, d_index, d_sign, batch)
        want = pm.apply_map(start, recs, coef, table, index=index, sign=sign, count=batch, ncmd=ncmd)
        same_bits(params, want)
        written = ~np.isnan(want)
        assert not written[batch:].any(), name
        assert written[:batch].any(axis=0).sum() == min(nrecs, max(n_params - 1, 1)), name
    # cmd_stride == 0: the launch shares row 0 of the table, whatever the index says
    params = torch.as_tensor(start, device="cuda")
    launch(torch, params, d_recs, d_coef, d_table, 0, ncmd, torch.as_tensor(cases["picked from a table"], device="cuda"),
           d_sign, batch)
    same_bits(params, pm.apply_map(start, recs, coef, table[0, :ncmd], sign=sign, count=batch))
    # fewer instances than rows written before: the rest keeps what the last launch left
    if batch > 1:
        before = params.cpu().numpy()
        launch(torch, params, d_recs, d_coef, d_table, stride, ncmd, None, d_sign, batch // 2)
        same_bits(params, pm.apply_map(before, recs, coef, table, sign=sign, count=batch // 2, ncmd=ncmd))


def test_signs_and_constants_are_rounded_one_by_one(torch_gpu):
    """Values whose fused product-sum differs from the product rounded first: c0 + (c1 * s) * x with a product
    that is not exact and a sum that cancels its leading bits."""
    torch = torch_gpu
    rng = np.random.default_rng(9)
    batch = 513
    recs = np.array([[0, 0, pm.CONST, 0], [1, 1, pm.SIGNED | pm.CONST, 0], [2, 0, pm.SIGNED, 0]], dtype=np.int32)
    coef = np.array([[-1.0, 1.0 + 2.0 ** -30], [-1.0, 1.0 - 2.0 ** -29], [0.0, -1.0]])    # (the sums cancel)
    cmd = 1.0 + rng.integers(1, 2 ** 20, (batch, 2)) * 2.0 ** -45        # (products need more than 53 bits)
    sign = rng.choice([-1.0, 1.0], batch)
    start = nan_payloads(batch, 4)
    params = torch.as_tensor(start, device="cuda")
    launch(torch, params, torch.as_tensor(recs, device="cuda"), torch.as_tensor(coef, device="cuda"),
           torch.as_tensor(cmd, device="cuda"), 2, 2, None, torch.as_tensor(sign, device="cuda"), batch)
    want = pm.apply_map(start, recs, coef, cmd, sign=sign)
    same_bits(params, want)
    assert np.array_equal(want[:, 2], -sign * cmd[:, 0])                    # (+-1: the host's product exactly)
    from fractions import Fraction
    fused = np.array([float(Fraction(coef[0, 1]) * Fraction(x) + Fraction(coef[0, 0])) for x in cmd[:, 0]])
    assert (fused != want[:, 0]).any()          # (the case does tell the two roundings apart)


# ---- 7. records out of range ----------------------------------------------------------------------------
def test_records_out_of_range_write_nothing(torch_gpu):
    torch = torch_gpu
    n_params, ncmd, batch = 11, 3, 70
    recs = np.array([[2, 0, 0, 0], [-1, 0, 0, 0], [5, 1, pm.CONST, 0], [n_params, 1, 0, 0], [7, 2, pm.SIGNED, 0],
                     [8, ncmd, 0, 0], [9, 0, 4, 0], [10, 1, pm.SIGNED | 8, 0], [0, 2, pm.SIGNED | pm.CONST, 0],
                     [3, -1, 0, 0], [4, 0, -1, 0]], dtype=np.int32)
    rng = np.random.default_rng(4)
    coef = rng.normal(0, 1, (len(recs), 2))
    cmd = rng.normal(0, 1, (batch, ncmd))
    sign = rng.choice([-1.0, 1.0], batch)
    start = nan_payloads(batch + EXTRA_ROWS, n_params)
    d = lambda a: torch.as_tensor(a, device="cuda")
    params = d(start)
    launch(torch, params, d(recs), d(coef), d(cmd), ncmd, ncmd, None, d(sign), batch)
    want = pm.apply_map(start, recs, coef, cmd, sign=sign, count=batch)
    same_bits(params, want)
    written = ~np.isnan(want[:batch]).all(axis=0)
    assert np.flatnonzero(written).tolist() == [0, 2, 5, 7]                 # the valid neighbours, and only they
    # without signs a SIGNED record is an unknown one: only the plain records write
    params = d(start)
    launch(torch, params, d(recs), d(coef), d(cmd), ncmd, ncmd, None, None, batch)
    want = pm.apply_map(start, recs, coef, cmd, sign=None, count=batch)
    same_bits(params, want)
    assert np.flatnonzero(~np.isnan(want[:batch]).all(axis=0)).tolist() == [2, 5]


# ---- 8. through the assembler: a graph, and no trip to the host -----------------------------------------------
def test_a_captured_map_follows_the_commands_and_reads_nothing_back(gpu_api, torch_gpu):
    torch = torch_gpu
    from mpcasm.engine import Assembler
    from mpcasm.walkers import COMMAND_COLUMNS, biped_command_rules

    conf = problems.BipedConfig(step_samples=8)
    form = problems.biped(gpu_api, conf)
    form.update(step_times=np.array([0, 8]), step_count=0)
    B, count, walkers = 96, 70, 150
    asm = Assembler(form, batch=B)
    pmap = asm.param_map(biped_command_rules(form), COMMAND_COLUMNS)
    assert pmap.nrecs == 18 and pmap.signed and pmap.ncmd == 4
    rng = np.random.default_rng(21)
    cmd_h = rng.normal(0, 0.3, (walkers, 4))
    idx = rng.permutation(walkers)[:count].astype(np.int32)
    sign_h = rng.choice([-1.0, 1.0], count)
    commands, index, sign = (torch.as_tensor(a, device="cuda") for a in (cmd_h, idx, sign_h))
    start = asm.params.cpu().numpy()
    with pytest.raises(ValueError):
        asm.apply_param_map(pmap, commands, index=index, count=count)          # signed records, no sign
    with pytest.raises(ValueError):
        asm.apply_param_map(pmap, commands.float(), index=index, sign=sign, count=count)
    with pytest.raises(ValueError):
        asm.apply_param_map(pmap, commands, index=np.array([walkers] + list(idx[1:])), sign=sign, count=count)
    assert np.array_equal(asm.params.cpu().numpy(), start)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = asm.apply_param_map(pmap, commands, index=index, sign=sign, count=count)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out is asm.params
    want = pm.apply_map(start, pmap.host_recs, pmap.host_coef, cmd_h, index=idx, sign=sign_h, count=count)
    same_bits(asm.params, want)
    assert (want[:count] != start[:count]).any(axis=0).sum() == 18 and np.array_equal(want[count:], start[count:])
    # captured once; a replay after the commands changed in place gives the new values
    other = torch.as_tensor(start, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        asm.apply_param_map(pmap, commands, index=index, sign=sign, count=count, params=other)
    cmd2 = rng.normal(0, 0.3, (walkers, 4))
    commands.copy_(torch.as_tensor(cmd2, device="cuda"))
    torch.cuda.set_sync_debug_mode("error")
    try:
        graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    same_bits(other, pm.apply_map(start, pmap.host_recs, pmap.host_coef, cmd2, index=idx, sign=sign_h, count=count))
    # one command row shared by the launch
    asm.apply_param_map(pmap, commands[5].contiguous(), sign=sign, count=count, params=other)
    same_bits(other, pm.apply_map(start, pmap.host_recs, pmap.host_coef, cmd2[5], sign=sign_h, count=count))
