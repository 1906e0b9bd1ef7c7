"""nerf_hugs_amd.hugs.SamImageEncoder (csrc/hugs_samencode.hip) against the restatement in tests/sam_encoder_ref.py run in float64.
Weights come from a seeded generator (non-zero rel_pos tables); nothing is downloaded.  depth 2: one windowed block (M = 4900
rows, pad keys) followed by one global block (flash form).

test_encode: the HIP output may differ from float64 by at most 4x what the same restatement in float32 on the CPU differs by (a
different fp32 summation order through the chained reductions); the yardstick is the CPU float32 run, never the HIP output.
Measured on an MI355X, max abs error (|ref| max | CPU float32 | HIP):
  D 128, 2 heads, (683, 1024) uint8     5.96 | 1.06e-5 | 2.72e-6      D 160, 2 heads, (683, 1024) uint8   5.99 | 1.35e-5 | 2.65e-6
  D 128, 2 heads, (1024, 1024) float32  5.31 | 9.91e-6 | 2.71e-6
("SAM image encoder"); the test prints the numbers for every case."""
import functools

import pytest
import torch

from tests import sam_encoder_ref as R

pytestmark = pytest.mark.gpu

# (D, heads, image (h, w), dtype): hd 64; hd 80 with D off the 64 tile; both with bottom padding, patch rows that straddle the
# pad edge (683 = 42 * 16 + 11) and all-pad patch rows; a full float32 image
CASES = [(128, 2, (683, 1024), torch.uint8), (160, 2, (683, 1024), torch.uint8), (128, 2, (1024, 1024), torch.float32)]


@functools.lru_cache(maxsize=None)
def _weights(D, heads):
  return R.make_weights(D, 2, heads, (1,), seed=D)


def _image(size, dtype):
  img = torch.randint(0, 256, (*size, 3), generator=torch.Generator().manual_seed(size[0]), dtype=torch.uint8)
  return img if dtype == torch.uint8 else img.float() + 0.25


@functools.lru_cache(maxsize=None)
def _encoder(D, heads):
  from nerf_hugs_amd import hugs
  return hugs.SamImageEncoder(_weights(D, heads))


@pytest.mark.parametrize('D,heads,size,dtype', CASES)
def test_encode(D, heads, size, dtype):
  w, img = _weights(D, heads), _image(size, dtype)
  ref = R.encode({k: v.double() for k, v in w.items()}, img)
  cpu = R.encode(w, img)
  got = _encoder(D, heads).encode(img.cuda())
  assert tuple(got.shape) == (256, 64, 64) and got.dtype == torch.float32 and got.is_cuda
  e_cpu, e_hip = float((cpu.double() - ref).abs().max()), float((got.cpu().double() - ref).abs().max())
  print(f'D={D} heads={heads} image={size} {dtype}: |ref| max {float(ref.abs().max()):.3g}, CPU float32 err {e_cpu:.3e}, HIP err {e_hip:.3e}')
  assert e_hip <= 4 * e_cpu, (e_hip, e_cpu)


def test_encode_is_deterministic():
  enc, img = _encoder(128, 2), _image((683, 1024), torch.uint8).cuda()
  assert torch.equal(enc.encode(img), enc.encode(img))


@pytest.mark.parametrize('key,change', [('blocks.0.attn.qkv.weight', None), ('blocks.0.attn.rel_pos_h', 25)])
def test_bad_weights_raise_value_error(key, change):
  from nerf_hugs_amd import hugs
  w = dict(_weights(128, 2))
  if change is None:
    del w[R.IE + key]
  else:
    w[R.IE + key] = w[R.IE + key][:change]
  with pytest.raises(ValueError, match=key.replace('.', r'\.')):
    hugs.SamImageEncoder(w)


def test_set_image_from_is_encode_then_set_image():
  from nerf_hugs_amd import hugs
  from tests import sam_decoder_ref
  enc, img, size = _encoder(128, 2), _image((683, 1024), torch.uint8).cuda(), (200, 300)
  pts = torch.tensor([[[40., 30.]], [[250., 150.]]]).cuda()
  a = hugs.SamPointDecoder(sam_decoder_ref.make_weights(0)).set_image_from(enc, img, size).predict(pts)
  b = hugs.SamPointDecoder(sam_decoder_ref.make_weights(0)).set_image(enc.encode(img), size).predict(pts)
  assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool(torch.isfinite(a[0]).all())
