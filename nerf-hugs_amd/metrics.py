"""The body of the reference's repository-level metrics.py (:36-89, run by scripts/metrics_*.sh) on the device: score the
`<experiment_dir>/<scene>/test_preds/*_gt.png` / `*_color.png` pairs that eval writes and report PSNR / SSIM / LPIPS per
image, per scene and overall, in the reference's nested dict and `metrics_results.json`.

  python -m nerf_hugs_amd.metrics --experiment_dir EXP --scene_names a b --save --alexnet alexnet.pth --lpips_lin alex.pth

psnr is image.mse -> PSNR, lpips is image.LpipsAlex (metrics.py:30-34,61; fp32 HIP kernels, from the two local weight files:
torchvision's AlexNet state dict and the lpips package's alex.pth; without them the 'lpips' entries are left out).
ssim is this package's existing dm_pix-form kernel (image.ssim: 11-tap Gaussian, 'valid' filtering); the reference's
metrics.py uses torchmetrics' StructuralSimilarityIndexMeasure, and the equality of the two is NOT pinned by a test
(torchmetrics is not a dependency of this package)."""
import argparse
import collections
import json
import os

import numpy as np
import torch

from .internal import image

IMAGE_TYPES = ['whole', 'half_right', 'half_left']


def _load(path, device):
  from PIL import Image
  rgb = np.asarray(Image.open(path).convert('RGB'), np.float32) / np.float32(255)
  return torch.from_numpy(rgb).to(device).clip(0., 1.)


def score_experiment(experiment_dir, scene_names, image_type='whole', lpips=None, save=False, output_dir='output_metrics',
                     device='cuda'):
  """metrics.py:36-89.  `lpips`: an image.LpipsAlex or None.  Returns {scene: {image: {metric: value}, 'mean': {...}},
  'mean': {...}} with plain floats."""
  if image_type not in IMAGE_TYPES:
    raise ValueError(f'image_type must be one of {IMAGE_TYPES}, got {image_type!r}')
  results = collections.defaultdict(dict)
  experiment_mean = collections.defaultdict(list)
  for scene in scene_names:
    pred_dir = os.path.join(experiment_dir, scene, 'test_preds')
    scene_mean = collections.defaultdict(list)
    for gt_name in sorted(f for f in os.listdir(pred_dir) if f.endswith('_gt.png')):
      name = gt_name[:-len('_gt.png')]
      pred = _load(os.path.join(pred_dir, f'{name}_color.png'), device)
      gt = _load(os.path.join(pred_dir, gt_name), device)
      half = pred.shape[1] // 2
      if image_type == 'half_left':
        pred, gt = pred[:, :half], gt[:, :gt.shape[1] // 2]
      elif image_type == 'half_right':
        pred, gt = pred[:, half:], gt[:, gt.shape[1] // 2:]
      pred, gt = pred.contiguous(), gt.contiguous()
      m = {'psnr': float(image.mse_to_psnr(image.mse(pred, gt))), 'ssim': float(image.ssim(pred, gt))}
      if lpips is not None:
        m['lpips'] = float(lpips(pred, gt))
      results[scene][name] = m
      for key, val in m.items():
        scene_mean[key].append(val)
    results[scene]['mean'] = {key: float(np.mean(val)) for key, val in scene_mean.items()}
    for key, val in results[scene]['mean'].items():
      experiment_mean[key].append(val)
  results['mean'] = {key: float(np.mean(val)) for key, val in experiment_mean.items()}
  results = dict(results)
  width = max(len(k) for k in results)
  for scene in results:
    tmp = results['mean'] if scene == 'mean' else results[scene]['mean']
    print(f'{scene}: {" " * (width - len(scene))}' +
          ', '.join(f'{k}={tmp[k]:.2f}' if k == 'psnr' else f'{k}={tmp[k]:.3f}' for k in ('psnr', 'ssim', 'lpips') if k in tmp))
  if save:
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'metrics_results.json'), 'w') as fp:
      json.dump(results, fp, indent=4)
  return results


def main(argv=None):
  parser = argparse.ArgumentParser(description='PSNR / SSIM / LPIPS of the test renders of an experiment.')
  parser.add_argument('--experiment_dir', type=str, help='the experiment directory (holds one folder per scene)')
  parser.add_argument('--scene_names', nargs='+', type=str, help='the scenes to score')
  parser.add_argument('--output_dir', type=str, default='output_metrics', help='where --save writes metrics_results.json')
  parser.add_argument('--save', action='store_true', help='write the per-image results as JSON')
  parser.add_argument('--image_type', type=str, choices=IMAGE_TYPES, default=IMAGE_TYPES[0], help='score the whole image or one half of it')
  parser.add_argument('--device', type=str, default='cuda', help='the GPU to run on')
  parser.add_argument('--alexnet', type=str, default=None, help="torchvision's AlexNet state dict, a local file")
  parser.add_argument('--lpips_lin', type=str, default=None, help="the lpips package's alex.pth (its linear layers), a local file")
  args = parser.parse_args(argv)
  if (args.alexnet is None) != (args.lpips_lin is None):
    parser.error('--alexnet and --lpips_lin go together')
  lpips = image.LpipsAlex.from_files(args.alexnet, args.lpips_lin, args.device) if args.alexnet else None
  score_experiment(args.experiment_dir, args.scene_names, args.image_type, lpips, args.save, args.output_dir, args.device)


if __name__ == '__main__':
  main()
