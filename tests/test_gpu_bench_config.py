"""The BENCHMARKED configurations at size (BASELINE.json configs[1..3]):
  (i)   8x1024 + 4x256 nets, fp32 MFMA mode, 64 rays: the full step against the oracle at 1e-4;
  (ii)  bf16, 1024 rays x (64+128) -- exactly what bench.py times: finite, bit-reproducible, weights sum to 1,
        the loss goes down over 20 steps, rendered colour within 2e-2 of the fp32 mode on the same weights;
  (iii) configs[2] (static masks, GLO 48, charb) at 4096 rays and configs[3]'s full combination (RobustNeRF 0.8 +
        contract + reciprocal + GLO 4, 16x16 patches) at 1024 rays per GPU: per-ray outputs against the oracle on
        a ray subsample, and the whole-batch losses recomputed by the oracle's loss functions from the product's
        own renderings (the normalisers span the batch, so the loss cannot be checked on a subsample)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDE = ["Config.data_loss_type = 'mse'", "Config.distortion_loss_mult = 0.01", "Model.opaque_background = True",
        "Model.num_levels = 2", "Model.num_prop_samples = 64", "Model.num_nerf_samples = 128", "PropMLP.net_depth = 4",
        "PropMLP.net_width = 256", "PropMLP.disable_rgb = True", "NerfMLP.net_depth = 8", "NerfMLP.net_width = 1024",
        "Config.randomized = True"]


def test_fp32_full_width_64_rays_full_step_vs_oracle():
  from tests.test_gpu_train_step import _run_case
  _run_case(["Config.patch_size = 8"] + WIDE)


def _bench_like(compute_dtype, seed=7):
  import bench
  from tests import hugs_testlib as H
  return H.make_pair(bench.GIN + ["Config.randomized = True"], seed=seed, compute_dtype=compute_dtype)


def test_bf16_1024_rays_step_properties():
  import bench
  runs = []
  for rep in range(2):
    config, model, state, _, train_step, cfg, oparams = _bench_like('bf16')
    batch = bench.synth_batch(4, 16, 5, 'cuda')
    gen = torch.Generator(device='cuda').manual_seed(123)
    losses = []
    for i in range(20):
      state, stats, gen = train_step(gen, state, batch, i / 20, None)
      losses.append(float(stats['loss']))
      assert np.isfinite(losses[-1]) and all(np.isfinite(float(v)) for v in stats['grad_norms'].values())
      assert all(np.isfinite(float(v)) for v in stats['opt_update_norms'].values())
    torch.cuda.synchronize()
    runs.append((state.flat.clone(), losses, model, state))
  assert torch.equal(runs[0][0], runs[1][0]), 'two identical runs differ: the step is not bit-reproducible'
  assert runs[0][1] == runs[1][1]
  losses = runs[0][1]
  assert np.mean(losses[-3:]) < 0.8 * np.mean(losses[:3]), losses
  # forward on the trained weights: weights of every ray sum to 1 (opaque background), bf16 vs fp32 mode
  model, state = runs[0][2], runs[0][3]
  from nerf_hugs_amd.internal import models as M
  batch = bench.synth_batch(4, 16, 5, 'cuda')
  eng = model.engine('cuda')
  r = M.rays_to_dict(batch.rays, 'cuda')
  lv = eng.forward(state.flat, r, 1.0, None, False)
  for l in lv:
    s = l['weights'].float().sum(-1)
    assert float((s - 1).abs().max()) < 2e-5
  rgb16 = lv[-1]['rgb_out'].clone()
  config32, model32, state32, _, _, _, _ = _bench_like('fp32')
  state32.flat.copy_(state.flat)
  eng32 = model32.engine('cuda')
  eng32.refresh_weights(state32.flat)
  rgb32 = eng32.forward(state32.flat, r, 1.0, None, False)[-1]['rgb_out']
  assert float((rgb16 - rgb32).abs().max()) < 2e-2
  assert float((rgb16 - rgb32).abs().mean()) < 3e-3


def _at_size(gin, n_patch, P, near, far, inlier, sub):
  from tests import hugs_testlib as H
  from oracle import torch_ref as R
  from nerf_hugs_amd.internal import models as M
  config, model, state, _, train_step, cfg, oparams = H.make_pair(gin, compute_dtype='fp32')
  batch = H.synth_rays(n_patch, P, 9, near=near, far=far)
  N, L = n_patch * P * P, model.num_levels
  g = torch.Generator(device='cuda').manual_seed(3)
  u01 = [torch.rand(N, generator=g, device='cuda') for _ in range(L)]
  eng = model.engine('cuda')
  eng.refresh_weights(state.flat)
  levels = eng.forward(state.flat, M.rays_to_dict(batch.rays, 'cuda'), 0.37, u01, False)
  pred = [lv['rgb_out'].cpu().clone() for lv in levels]
  hist = [dict(sdist=lv['sdist'].cpu().clone(), weights=lv['weights'].float().cpu().clone()) for lv in levels]
  # per-ray outputs on a subsample against the oracle
  rows = torch.arange(0, N, sub)
  orays = {k: v[rows] for k, v in H.oracle_rays(batch).items()}
  orend, ohist = R.model_forward(cfg, oparams, orays, 0.37, [u.cpu()[rows] for u in u01], False)
  for l in range(L):
    assert H.relerr(hist[l]['sdist'][rows], ohist[l]['sdist']) < 1e-4, f'sdist L{l}'
    assert float((hist[l]['weights'][rows] - ohist[l]['weights'].detach()).abs().max()) < 3e-4, f'weights L{l}'
    assert float((pred[l][rows] - orend[l]['rgb'].detach()).abs().max()) < 1e-4, f'rgb L{l}'
  # whole-batch losses from the product's own renderings, through the oracle's loss code
  thr = None if inlier is None else np.full((L, 1), inlier, np.float32)
  state, stats, _ = train_step(u01, state, batch, 0.37, thr)
  torch.cuda.synchronize()
  gt = batch.rgb.reshape(-1, 3)
  rend = [{'rgb': p} for p in pred]
  if cfg.transient_type == 'robustnerf':
    rs = [{'rgb': p.reshape(-1, P, P, 3)} for p in pred]
    data, st = R.compute_robustnerf_loss(cfg, gt.reshape(-1, P, P, 3), rs, [torch.tensor([inlier])] * L)
    for k in ('inlier_threshold', 'is_inlier_loss', 'has_inlier_neighbors', 'is_inlier_patch', 'mask'):
      np.testing.assert_allclose(stats['robust_' + k].numpy(), st['robust_' + k].numpy(), rtol=2e-5, atol=1e-6, err_msg=k)
  else:
    data, st = R.compute_data_loss(cfg, gt, H.oracle_rays(batch), rend, cfg.transient_type == 'withmask')
  assert abs(float(stats['losses']['data']) - float(data)) <= 2e-5 * abs(float(data))
  np.testing.assert_allclose(stats['mses'].numpy(), st['mses'].numpy(), rtol=2e-5)
  inter = float(R.interlevel_loss(cfg, hist))
  assert abs(float(stats['losses']['interlevel']) - inter) <= 2e-4 * abs(inter) + 1e-9
  dist = float(R.distortion_loss(cfg, hist))
  assert abs(float(stats['losses']['distortion']) - dist) <= 2e-5 * abs(dist) + 1e-10
  assert all(np.isfinite(float(v)) for v in stats['grad_norms'].values())


def test_cfg3_static_masks_glo48_charb_4096_rays():
  import bench
  _at_size(bench.GIN_CFG3 + ["Config.randomized = True"], 16, 16, (0.5, 1.0), 3.0, None, 64)


def test_cfg4_robustnerf_contract_reciprocal_glo4_1024_rays():
  import bench
  _at_size(bench.GIN_CFG4 + ["Config.randomized = True"], 4, 16, (0.05, 0.3), 1e6, 0.3, 16)


def test_bench_plain_run_one_window_and_reproducible_dump(tmp_path):
  """A plain `bench.py --gpus 1 --steps K --warmup W` run: one JSON line, ONE window of exactly K steps (`ms_per_step` and `value`
  are that window's), nothing of the --full legs in the line; --dump-outputs writes float32 / float64 .npy files of at most 64 MB
  in all -- the (state, stats, rng) that step W + K handed back -- and a second run with the same arguments writes the same bits
  (the inputs are seeded and the step is bit-reproducible: test_bf16_1024_rays_step_properties)."""
  import json
  import os
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  K, W = 3, 3          # (W = 3: two eager steps and the capture, so the timed steps are replays as in a real run)
  outs = []
  for tag in ('a', 'b'):
    d = str(tmp_path / tag)
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W),
                          '--batch-pool', '8', '--dump-outputs', d], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    outs.append((json.loads(lines[0]), d))
  line = outs[0][0]
  for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
    assert k in line, k
  assert line['steps'] == K and line['warmup'] == W and line['windows'] == 1 and line['unit'] == 'rays/s' and line['dtype'] == 'bf16'
  assert line['higher_is_better'] is True and line['value_min'] == line['value_max'] == line['value']
  assert abs(line['timed_s'] - K * line['ms_per_step'] * 1e-3) <= 1e-3            # the window IS the K steps (both rounded to 3 digits)
  assert abs(line['value'] - 1024 / (line['ms_per_step'] * 1e-3)) < 2e-3 * line['value']
  for k in ('roofline', 'instep_kernels', 'cpu_baseline'):
    assert k not in line, k
  for k in ('fixed_batch', 'random_targets', 'host_enqueue_ms_per_step', 'trunk_relu_active_fraction', 'eval_psnr_vs_cpu_fp32_db'):
    assert line[k] is None, k
  names = sorted(os.listdir(outs[0][1]))
  assert names == sorted(os.listdir(outs[1][1]))
  for n in ('params.npy', 'adam_m.npy', 'adam_v.npy', 'step.npy', 'rng.npy', 'stats.loss.npy', 'stats.psnr.npy', 'stats.mses.npy'):
    assert n in names, n
  total = 0
  for n in names:
    a, b = np.load(os.path.join(outs[0][1], n)), np.load(os.path.join(outs[1][1], n))
    assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert np.array_equal(a, b), f'{n}: two runs with the same arguments differ'
    total += os.path.getsize(os.path.join(outs[0][1], n))
  assert total <= 64 << 20
  assert float(np.load(os.path.join(outs[0][1], 'step.npy'))) == K + W
  assert float(np.load(os.path.join(outs[0][1], 'stats.loss.npy'))) == pytest.approx(line['loss_last'], abs=1e-6)
  assert np.abs(np.load(os.path.join(outs[0][1], 'adam_v.npy'))).max() > 0      # the state the steps updated, not its initial zeros


def test_bench_cfg5_plain_run_dump(tmp_path):
  """`bench.py --config cfg5 --dump-outputs`: the nerfacto step's set (packed stats, the final level's rgb and weights, parameters
  and Adam moments as seeded samples) is float32 / float64, finite and at most 64 MB in all, from ONE window of K steps.  (No
  run-to-run equality here: the table gradients are float atomics, whose order is not fixed.)"""
  import json
  import os
  import subprocess
  import sys
  import bench
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  d = str(tmp_path / 'cfg5')
  out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--config', 'cfg5', '--steps', '2', '--warmup', '2',
                        '--dump-outputs', d], capture_output=True, text=True, timeout=300, cwd=root)
  assert out.returncode == 0, out.stderr[-3000:]
  lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, out.stdout[-2000:]
  line = json.loads(lines[0])
  assert line['steps'] == 2 and line['windows'] == 1 and line['dtype'] == 'fp16' and line['ms_per_step'] > 0
  for k in ('roofline', 'instep_kernels', 'with_16bit_grid_input_gradient'):
    assert k not in line, k
  assert sorted(os.listdir(d)) == ['adam_m.npy', 'adam_v.npy', 'params.npy', 'rgb.npy', 'stats.npy', 'weights.npy']
  arrs = {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}
  for n, a in arrs.items():
    assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
  assert sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)) <= 64 << 20
  assert arrs['rgb'].shape == (16384, 3) and arrs['weights'].shape == (16384, 128) and arrs['stats'].shape == (16,)
  assert arrs['params'].shape == arrs['adam_m'].shape == arrs['adam_v'].shape == (bench.DUMP_CAP,)
  assert arrs['rgb'].min() >= -1e-3 and arrs['rgb'].max() <= 1 + 1e-3 and arrs['weights'].min() >= 0 and arrs['weights'].max() <= 1
  assert float(arrs['stats'][1]) == pytest.approx(line['loss_rgb_last'], abs=1e-6) and np.abs(arrs['adam_v']).max() > 0
