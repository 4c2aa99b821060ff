"""Guard the driver contract: `python bench.py --gpus N --steps K --warmup W`
must print exactly one JSON line with the required fields, single- and
multi-process (gloo on CPU)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ['--steps', '1', '--warmup', '0', '--points', '32', '--dim', '32',
        '--heads', '2', '--dim-head', '16', '--depth', '1',
        '--num-degrees', '2', '--num-neighbors', '4', '--dtype', 'fp32']

REQUIRED = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
            'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
            'dtype', 'data', 'config'}


def _check_line(out):
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, f'expected exactly one JSON line, got: {out!r}'
    d = json.loads(lines[0])
    assert REQUIRED <= set(d), REQUIRED - set(d)
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert d['config']['global_batch'] == d['n_gpus'] * 1
    return d


def test_bench_single_process():
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1'] + TINY,
                       capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _check_line(r.stdout)
    assert d['n_gpus'] == 1


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's loss, model output and gradient
    sample as float32 .npy files; the same arguments give the same inputs and
    the same sample layout on every run, and --full leaves the headline path
    untouched. CPU so that the arithmetic itself is run-to-run exact."""
    import numpy as np
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    dumps = []
    for name, extra in (('a', []), ('b', ['--full'])):
        d = tmp_path / name
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1'] + TINY
                           + ['--steps', '2', '--dump-outputs', str(d)] + extra,
                           capture_output=True, text=True, cwd=REPO,
                           timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert _check_line(r.stdout)['steps'] == 2
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    a, b = dumps
    assert set(a) == set(b) == {'loss.npy', 'out.npy', 'grad_sample.npy'}
    assert a['out.npy'].shape == (1, 32, 32) and a['loss.npy'].shape == (1,)
    assert a['grad_sample.npy'].size > 0 and a['grad_sample.npy'].any()
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert sum(v.nbytes for v in a.values()) <= 64 << 20
        assert np.array_equal(a[k], b[k]), k


def test_bench_two_process_gloo():
    # hide any GPU so setup_distributed picks gloo: two ranks cannot share
    # one device over nccl (this test exercises the CPU DP path everywhere)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    r = subprocess.run(
        [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', '29719', 'bench.py', '--gpus', '2'] + TINY,
        capture_output=True, text=True, cwd=REPO, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _check_line(r.stdout)
    assert d['n_gpus'] == 2 and d['config']['parallelism'] == 'dp2'


def test_denoise_example_runs():
    """The training example must run one accumulation cycle on CPU."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, 'examples/denoise.py', '--steps', '1',
                        '--length', '16'],
                       capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert 'loss:' in r.stdout


def test_infer_example_cpu_smoke():
    """examples/infer.py runs end-to-end on CPU (tiny config)."""
    import json
    import subprocess
    import sys
    out = subprocess.run(
        [sys.executable, 'examples/infer.py', '--points', '24', '--dim', '16',
         '--heads', '2', '--dim-head', '8', '--depth', '1',
         '--num-degrees', '2', '--num-neighbors', '4', '--iters', '1',
         '--warmup', '0', '--no-graph'],
        capture_output=True, text=True, timeout=300,
        cwd=__import__('os').path.dirname(__import__('os').path.dirname(
            __import__('os').path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    parsed = json.loads(out.stdout.strip().splitlines()[-1])
    assert parsed['samples_per_sec'] > 0


def test_denoise_checkpoint_resume(tmp_path):
    """Checkpoint then resume: second invocation must pick up at the saved
    step and run only the remaining steps."""
    import subprocess
    import sys
    ck = str(tmp_path / 'ck.pt')
    base = [sys.executable, 'examples/denoise.py', '--length', '12',
            '--checkpoint', ck, '--save-every', '1']
    r = subprocess.run(base + ['--steps', '1'], capture_output=True,
                       text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert (tmp_path / 'ck.pt').exists()
    r = subprocess.run(base + ['--steps', '2'], capture_output=True,
                       text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert 'resumed from' in r.stdout and 'at step 1' in r.stdout
    # exactly one more optimizer step ran
    assert r.stdout.count('loss:') == 1


def test_serve_app_in_process():
    """examples/serve.py app answers /health and /predict via the in-process
    test client (no socket)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'serve_example', os.path.join(REPO, 'examples', 'serve.py'))
    serve = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(serve)
    from fastapi.testclient import TestClient

    args = serve.parse_args(['--dim', '16', '--heads', '2', '--dim-head', '8',
                             '--depth', '1', '--num-neighbors', '4'])
    client = TestClient(serve.build_app(args))

    r = client.get('/health')
    assert r.status_code == 200 and r.json()['status'] == 'ok'

    import torch
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(12, 16, generator=g).tolist()
    coors = torch.randn(12, 3, generator=g).tolist()
    r = client.post('/predict', json={'feats': feats, 'coors': coors})
    assert r.status_code == 200, r.text
    body = r.json()
    assert len(body['output']) == 12 and len(body['output'][0]) == 16
    assert body['latency_ms'] > 0

    # shape validation is a 422, not a 500
    r = client.post('/predict', json={'feats': feats, 'coors': coors[:5]})
    assert r.status_code == 422


def test_bench_preset_with_explicit_override():
    """Preset values fill defaults but explicit flags win (bench.py preset
    precedence): --preset qm9 sets points=29/batch=16, an explicit --batch 2
    overrides the preset's 16."""
    import json
    import subprocess
    import sys
    r = subprocess.run(
        [sys.executable, 'bench.py', '--preset', 'qm9', '--steps', '1',
         '--warmup', '0', '--batch', '2', '--depth', '1'],
        capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    cfg = d['config']
    assert cfg['points'] == 29          # from the preset
    assert cfg['global_batch'] == 2     # explicit flag beat the preset's 16
    assert cfg['depth'] == 1            # explicit flag beat the preset's 4
    assert d['metric'].endswith('preset=qm9')


def test_serve_loads_checkpoint(tmp_path, monkeypatch):
    """serve.py --checkpoint actually loads the weights: predictions from a
    server started on a saved checkpoint differ from random init and equal
    a direct forward of the checkpointed model."""
    import importlib.util
    import torch
    # the comparison below is against an fp32 CPU forward at atol=1e-5, so
    # the server must take its CPU path too, also where a GPU is present
    # (there it would otherwise answer from the bf16 autocast path)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    spec = importlib.util.spec_from_file_location(
        'serve_example2', os.path.join(REPO, 'examples', 'serve.py'))
    serve = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(serve)
    from fastapi.testclient import TestClient

    flags = ['--dim', '16', '--heads', '2', '--dim-head', '8',
             '--depth', '1', '--num-neighbors', '4']
    args = serve.parse_args(flags)

    # make a model with DIFFERENT weights than serve's seed-0 init
    # (build_model seeds itself, so perturb after construction)
    ref = serve.build_model(serve.parse_args(flags), torch.device('cpu'))
    with torch.no_grad():
        for p_ in ref.parameters():
            p_.add_(torch.randn_like(p_) * 0.05)
    ck = tmp_path / 'ck.pt'
    torch.save({'model': ref.state_dict(), 'step': 7}, ck)

    g = torch.Generator().manual_seed(9)
    feats = torch.randn(12, 16, generator=g)
    coors = torch.randn(12, 3, generator=g)
    body = {'feats': feats.tolist(), 'coors': coors.tolist()}

    plain = TestClient(serve.build_app(args)).post('/predict', json=body)
    loaded = TestClient(serve.build_app(
        serve.parse_args(flags + ['--checkpoint', str(ck)]))) \
        .post('/predict', json=body)
    assert plain.status_code == 200 and loaded.status_code == 200
    out_loaded = torch.tensor(loaded.json()['output'])
    assert not torch.allclose(torch.tensor(plain.json()['output']),
                              out_loaded)                   # weights changed
    with torch.inference_mode():
        want = ref(feats.unsqueeze(0), coors.unsqueeze(0),
                   torch.ones(1, 12, dtype=torch.bool), return_type=0)
    assert torch.allclose(out_loaded, want.squeeze(0), atol=1e-5)
