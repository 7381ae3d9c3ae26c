"""bench.py command line: the contract flags exist and --help renders (argparse %-formats every help string); the self-launch
builds exactly the driver's `torch.distributed.run` command line and refuses when GPUs are missing; the rank check sees the
real process group (2 gloo ranks)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_renders_and_names_the_contract_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-400:]
    for flag in ('--gpus', '--steps', '--warmup', '--storage', '--mode', '--full', '--dump-outputs'):
        assert flag in r.stdout, flag


def _bench():
    import importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module('bench')


def test_self_launch_builds_the_drivers_command_line(monkeypatch):
    """`python bench.py --gpus N` without a launcher runs itself as a child
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <flags>`
    and exits with its status (tools/dist_train.sh:10-20 is the reference's launcher); under a launcher, or for one GPU, it
    does nothing."""
    import subprocess
    import torch
    bench = _bench()
    argv = ['--gpus', '4', '--steps', '7', '--warmup', '2', '--mode', 'train']
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 8)
    seen = {}

    def fake_call(cmd):
        seen['cmd'] = cmd
        return 3
    monkeypatch.setattr(subprocess, 'call', fake_call)
    args = bench.parse()
    try:
        bench.self_launch(args)
        raise AssertionError('expected the exit status of the child')
    except SystemExit as e:
        assert e.code == 3
    cmd = seen['cmd']
    assert cmd[0] == sys.executable
    assert cmd[1:5] == ['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=4']
    assert cmd[5:7] == ['--master-addr', '127.0.0.1'] and cmd[7] == '--master-port' and 1024 < int(cmd[8]) < 65536
    assert cmd[9] == os.path.join(ROOT, 'bench.py') and cmd[10:] == argv
    # fewer GPUs than ranks: refused before anything is launched
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 2)
    seen.clear()
    try:
        bench.self_launch(args)
        raise AssertionError('expected a refusal')
    except SystemExit as e:
        assert 'only 2 GPU(s) visible' in str(e.code) and not seen
    # under a launcher (WORLD_SIZE set) and for --gpus 1: no-op
    monkeypatch.setenv('WORLD_SIZE', '4')
    assert bench.self_launch(args) is None and not seen
    monkeypatch.delenv('WORLD_SIZE')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1'])
    assert bench.self_launch(bench.parse()) is None and not seen


def test_plain_run_is_lean_and_full_keeps_the_legs(monkeypatch):
    """A plain run times the headline only; --full turns the extra legs back on (and the --no-* flags still parse)."""
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--full', '--no-cpu-baseline', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full is True and a.no_cpu_baseline and a.dump_outputs == 'out'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    try:
        bench.parse()
        raise AssertionError('--steps 0 accepted')
    except SystemExit as e:
        assert e.code == 2


def test_dump_outputs_writes_seeded_float_arrays(tmp_path):
    """--dump-outputs: float32 / float64 .npy files; an output larger than DUMP_SAMPLE is kept as a fixed seeded sample with its
    positions, the same from call to call; more than DUMP_LIMIT bytes in all is refused."""
    import numpy as np
    import torch
    bench = _bench()
    g = torch.Generator().manual_seed(1)
    vol = torch.randn(2, 3, 4, 5, 6, generator=g).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / 'small'), bench.volume_outputs(vol))
    whole = np.load(tmp_path / 'small' / 'bev_volume.npy')
    sums = np.load(tmp_path / 'small' / 'bev_volume_sum_bc.npy')
    assert whole.dtype == np.float32 and np.array_equal(whole, vol.float().reshape(-1).numpy())
    assert sums.dtype == np.float64 and sums.shape == (2, 3)
    assert np.allclose(sums, vol.double().sum(dim=(2, 3, 4)).numpy(), rtol=0, atol=1e-9)
    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32).reshape(1, 1, 3, 1, -1)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), bench.volume_outputs(big))
    sa, sb = (np.load(tmp_path / d / 'bev_volume_sample.npy') for d in ('a', 'b'))
    pos = np.load(tmp_path / 'a' / 'bev_volume_sample_positions.npy')
    assert sa.shape == (bench.DUMP_SAMPLE,) and np.array_equal(sa, sb)
    assert pos.dtype == np.float64 and np.array_equal(sa, pos.astype(np.float32))
    assert not (tmp_path / 'a' / 'bev_volume.npy').exists()
    try:
        bench.dump_outputs(str(tmp_path / 'c'), {'x': torch.zeros(bench.DUMP_LIMIT // 4 + 1)})
        raise AssertionError('oversized dump accepted')
    except SystemExit as e:
        assert 'more than' in str(e.code) and not (tmp_path / 'c').exists()


def test_train_outputs_sample_params_and_grads():
    bench = _bench()
    import torch
    ps = [torch.nn.Parameter(torch.full((3, 2), float(i))) for i in range(3)]
    ps[0].grad = torch.ones(3, 2)
    res = bench.train_outputs(torch.tensor(2.5), ps)
    assert res['loss'].tolist() == [2.5]
    assert res['param_sum_per_tensor'].tolist() == [0.0, 6.0, 12.0] and res['grad_sum_per_tensor'].tolist() == [6.0, 0.0, 0.0]
    assert res['param'].tolist() == [0.0] * 6 + [1.0] * 6 + [2.0] * 6 and res['grad'].tolist() == [1.0] * 6 + [0.0] * 12
    big = torch.nn.Parameter(torch.arange(bench.DUMP_SAMPLE + 5, dtype=torch.float32))
    big.grad = -big.detach()
    res = bench.train_outputs(torch.tensor(0.0), [big])
    pos = res['param_sample_positions']
    assert sorted(res) == ['grad_sample', 'grad_sum_per_tensor', 'loss', 'param_sample', 'param_sample_positions', 'param_sum_per_tensor']
    assert pos.dtype == torch.float64 and torch.equal(res['param_sample'].double(), pos) and torch.equal(res['grad_sample'].double(), -pos)


@pytest.mark.gpu
def test_plain_run_prints_the_line_and_dumps_the_last_steps_volume(tmp_path):
    """A plain run on a small config: one JSON line with the headline fields, exactly --steps timed steps, none of the --full
    legs, and DIR/bev_volume.npy = the volume the view transformer computes from the same seeded inputs."""
    import numpy as np
    import torch
    from fb_bev_amd import shard, synthetic as S
    from fb_bev_amd.view_transformer import LSSViewTransformerFunction3D
    d = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--config', 'SMALL', '--batch', '2', '--dump-outputs', str(d)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res['unit'] == 'samples/s' and res['higher_is_better'] is True and res['dtype'] == 'f32'
    assert res['steps'] == 3 and res['full'] is False and res['value'] > 0 and res['ms_per_step'] > 0
    assert abs(res['value'] - 2 / (res['ms_per_step'] * 1e-3)) <= 1e-6 * res['value']
    for leg in ('cpu_baseline', 'bf16_storage', 'pipelined', 'index_cache', 'fb_projection', 'reference_same_gpu'):
        assert leg not in res, leg
    vol = np.load(d / 'bev_volume.npy')
    sums = np.load(d / 'bev_volume_sum_bc.npy')
    assert vol.dtype == np.float32 and sums.dtype == np.float64
    dev = torch.device('cuda:0')
    cfg = S.CONFIGS['SMALL']
    cam = [t.to(dev) for t in S.camera_rig(cfg, 2, seed=shard.shard_seed(0), bda_aug=True)]
    depth, ctx = (t.to(dev) for t in S.depth_and_context(cfg, 2, seed=shard.shard_seed(0)))
    vt = LSSViewTransformerFunction3D(cfg.grid_config, cfg.input_size, cfg.downsample).to(dev)
    with torch.no_grad():
        exp = vt(cam, ctx, depth).permute(0, 1, 4, 2, 3).contiguous().cpu()     # (B, C, Z, Y, X), the volume bench.py times
    assert vol.shape == (exp.numel(),)
    assert np.allclose(vol, exp.reshape(-1).numpy(), rtol=1e-5, atol=1e-5)
    assert np.allclose(sums, exp.double().sum(dim=(2, 3, 4)).numpy(), rtol=1e-6, atol=1e-4)


def _rank_check_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    import types
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import bench
    dist.init_process_group('gloo')
    cpu = torch.device('cpu')
    ok = bench.check_ranks(types.SimpleNamespace(gpus=2), world, rank, cpu, index=rank)
    res = [ok]
    for gpus, index in ((4, rank), (2, 0)):          # --gpus disagrees with the group; two ranks on one device
        try:
            bench.check_ranks(types.SimpleNamespace(gpus=gpus), world, rank, cpu, index=index)
            res.append('accepted')
        except SystemExit as e:
            res.append(str(e.code))
    q.put((rank, res))
    dist.destroy_process_group()


def test_rank_check_sees_the_process_group():
    """`rccl_ranks` / `rank_devices` of the JSON line come from the process group itself (2 gloo ranks here): size ==
    --gpus, one device per rank; a mismatch or a shared device ends the run instead of reporting a wrong n_gpus."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_check_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        ok, wrong_n, shared = res[r]
        assert ok == (2, [0, 1])
        assert 'the process group has 2 rank(s)' in wrong_n
        assert 'share a device' in shared
