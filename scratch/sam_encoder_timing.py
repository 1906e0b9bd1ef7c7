"""One vit_h-shaped image encode (D 1280, depth 32, 16 heads, global blocks 7 / 15 / 23 / 31, random weights): hugs.SamImageEncoder
against the float32 restatement of tests/sam_encoder_ref.py on the same GPU (torch on rocBLAS).
  python scratch/sam_encoder_timing.py time  <out.txt>   event-timed, HIP and torch alternated: 2 warm-up calls, median of 5 windows
  python scratch/sam_encoder_timing.py hip               1 warm-up + 3 encodes, to run under rocprofv3 --kernel-trace -f csv
  python scratch/sam_encoder_timing.py stats <trace dir> <out.txt>   per-kernel times of that trace (per encode) appended to out.txt"""
import collections
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, DEPTH, HEADS, GLOBAL = 1280, 32, 16, (7, 15, 23, 31)
HD = D // HEADS
NWIN = DEPTH - len(GLOBAL)


def gemm_flops():
  """2 M N K of every k_enc_gemm launch of one encode (rel-pos products included)."""
  f = 2 * 4096 * 768 * D + 2 * 4096 * D * 256 + 2 * 4096 * 2304 * 256
  for rows, pw, n in ((4900, 64, NWIN), (4096, 256, len(GLOBAL))):
    f += n * (2 * rows * D * 3 * D + 2 * rows * D * D + 2 * 2 * 4096 * D * 4 * D + 2 * rows * HD * pw * HEADS)
  return f


def timed(fn, n=1):
  import torch
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(n):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / n


def setup():
  import torch
  from nerf_hugs_amd import hugs
  from tests import sam_encoder_ref as R
  w = R.make_weights(D, DEPTH, HEADS, GLOBAL, seed=0)
  enc = hugs.SamImageEncoder(w)
  img = torch.randint(0, 256, (683, 1024, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
  return torch, R, w, enc, img


def main():
  mode = sys.argv[1]
  if mode == 'stats':
    f = glob.glob(f'{sys.argv[2]}/**/*kernel_trace.csv', recursive=True)[0]
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
      if 'k_enc_' in r['Kernel_Name']:
        name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        agg[name].append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    n_enc = 4
    with open(sys.argv[3], 'a') as out:
      out.write(f'HIP kernels, rocprofv3 --kernel-trace in a run of its own, ms per encode (mean of {n_enc} encodes):\n')
      for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        out.write(f'  {k}: {sum(v) / 1e6 / n_enc:.2f} ms in {len(v) // n_enc} launches\n')
      gemm = sum(sum(v) for k, v in agg.items() if 'k_enc_gemm' in k) / 1e9 / n_enc
      out.write(f'  all k_enc_gemm: {gemm * 1e3:.2f} ms for {gemm_flops() / 1e12:.2f} TFLOP = {gemm_flops() / gemm / 1e12:.1f} TFLOP/s\n')
    return
  torch, R, w, enc, img = setup()
  if mode == 'hip':
    for _ in range(4):
      enc.encode(img)
    torch.cuda.synchronize()
    return
  wd = {k: v.cuda() for k, v in w.items()}
  g = torch.Generator(device='cuda').manual_seed(2)
  rn = lambda *s: torch.randn(*s, generator=g, device='cuda')
  b0, b7 = R.IE + 'blocks.0.', R.IE + 'blocks.7.'
  qkv_w, qkv_g = [rn(25, HEADS, 196, HD) for _ in range(3)], [rn(1, HEADS, 4096, HD) for _ in range(3)]
  y_w, y_g, h = rn(4900, D), rn(4096, D), rn(4096, 4 * D)
  lin = lambda x, b, name: torch.nn.functional.linear(x, wd[b + name + '.weight'], wd[b + name + '.bias'])
  legs = {
      'HIP encode': lambda: enc.encode(img),
      'torch encode': lambda: R.encode(wd, img),
      'torch global attention core (one block)': lambda: R.attention_core(*qkv_g, wd[b7 + 'attn.rel_pos_h'], wd[b7 + 'attn.rel_pos_w'], 64),
      'torch windowed attention core (one block)': lambda: R.attention_core(*qkv_w, wd[b0 + 'attn.rel_pos_h'], wd[b0 + 'attn.rel_pos_w'], 14),
      'torch linear layers of a windowed block (qkv, proj, lin1, lin2)':
          lambda: (lin(y_w, b0, 'attn.qkv'), lin(y_w, b0, 'attn.proj'), lin(y_g, b0, 'mlp.lin1'), lin(h, b0, 'mlp.lin2')),
  }
  with torch.no_grad():
    for fn in legs.values():
      for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = collections.defaultdict(list)
    for _ in range(5):
      for name, fn in legs.items():
        times[name].append(timed(fn))
    err = float((enc.encode(img) - R.encode(wd, img)).abs().max())
  with open(sys.argv[2], 'w') as out:
    out.write(f'{torch.cuda.get_device_name(0)}; one image encode at the vit_h shape (D {D}, depth {DEPTH}, {HEADS} heads), (683, 1024) uint8 image; '
              'ms, median (min..max) of 5 alternated event-timed windows after 2 warm-up calls\n')
    for name, v in times.items():
      out.write(f'{name}: {statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})\n')
    lin_ms = statistics.median(times['torch linear layers of a windowed block (qkv, proj, lin1, lin2)'])
    blk = 2 * 4900 * D * 4 * D + 2 * 2 * 4096 * D * 4 * D
    out.write(f'torch linear layers: {blk / 1e12:.3f} TFLOP per windowed block = {blk / lin_ms / 1e9:.1f} TFLOP/s\n')
    out.write(f'max |HIP - torch float32| of the two encodes: {err:.3e}\n')


if __name__ == '__main__':
  main()
