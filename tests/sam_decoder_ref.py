"""A plain PyTorch restatement of segment_anything's point prompt encoder + mask decoder (multimask output) and of
postprocess_masks, in the dtype of the weights it is given (the tests run it in float64 and, for the tolerance, in float32 on the
CPU).  A helper for tests/test_gpu_sam_decoder.py, not a test.  Keys are those of a segment_anything checkpoint."""
import math

import torch
import torch.nn.functional as F

PE, MD = 'prompt_encoder.', 'mask_decoder.'
TR = MD + 'transformer.'


def make_weights(seed=0):
  """A checkpoint-shaped dict of float32 tensors from a seeded generator: linear / conv weights scaled by 1/sqrt(fan_in), small
  biases, LayerNorm gains near 1, unit-scale embeddings."""
  g = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=g)
  w = {PE + 'pe_layer.positional_encoding_gaussian_matrix': rn(2, 128), PE + 'not_a_point_embed.weight': rn(1, 256),
       PE + 'point_embeddings.0.weight': rn(1, 256), PE + 'point_embeddings.1.weight': rn(1, 256),
       PE + 'no_mask_embed.weight': rn(1, 256), MD + 'iou_token.weight': rn(1, 256), MD + 'mask_tokens.weight': rn(4, 256)}

  def lin(name, cin, cout):
    w[name + '.weight'], w[name + '.bias'] = rn(cout, cin) / math.sqrt(cin), 0.1 * rn(cout)

  def norm(name, c):
    w[name + '.weight'], w[name + '.bias'] = 1 + 0.1 * rn(c), 0.1 * rn(c)

  def attn(name, inner):
    for p in 'qkv':
      lin(f'{name}.{p}_proj', 256, inner)
    lin(name + '.out_proj', inner, 256)

  for i in range(2):
    L = f'{TR}layers.{i}.'
    attn(L + 'self_attn', 256), attn(L + 'cross_attn_token_to_image', 128), attn(L + 'cross_attn_image_to_token', 128)
    lin(L + 'mlp.lin1', 256, 2048), lin(L + 'mlp.lin2', 2048, 256)
    for j in range(1, 5):
      norm(f'{L}norm{j}', 256)
  attn(TR + 'final_attn_token_to_image', 128), norm(TR + 'norm_final_attn', 256)
  w[MD + 'output_upscaling.0.weight'], w[MD + 'output_upscaling.0.bias'] = rn(256, 64, 2, 2) / 16, 0.1 * rn(64)
  norm(MD + 'output_upscaling.1', 64)
  w[MD + 'output_upscaling.3.weight'], w[MD + 'output_upscaling.3.bias'] = rn(64, 32, 2, 2) / 8, 0.1 * rn(32)
  for name, cout in [(f'{MD}output_hypernetworks_mlps.{m}', 32) for m in range(4)] + [(MD + 'iou_prediction_head', 4)]:
    lin(name + '.layers.0', 256, 256), lin(name + '.layers.1', 256, 256), lin(name + '.layers.2', 256, cout)
  return w


def pos_enc(G, c):
  v = (2 * c - 1) @ G * (2 * math.pi)
  return torch.cat([v.sin(), v.cos()], -1)


def _attn(w, name, q, k, v):
  q, k, v = (F.linear(x, w[f'{name}.{p}_proj.weight'], w[f'{name}.{p}_proj.bias']) for x, p in ((q, 'q'), (k, 'k'), (v, 'v')))
  heads = lambda x: x.reshape(x.shape[0], x.shape[1], 8, -1).transpose(1, 2)
  q, k, v = heads(q), heads(k), heads(v)
  a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]), -1) @ v
  return F.linear(a.transpose(1, 2).flatten(2), w[name + '.out_proj.weight'], w[name + '.out_proj.bias'])


def _mlp3(w, name, x):
  for i in range(3):
    x = F.linear(x, w[f'{name}.layers.{i}.weight'], w[f'{name}.layers.{i}.bias'])
    x = F.relu(x) if i < 2 else x
  return x


def decode(w, embedding, coords, labels, ln_eps=1e-5):
  """embedding [256,64,64]; coords [N,P,2] xy in model-input pixels; labels [N,P] in {0,1}.  -> lowres [N,3,256,256], iou [N,3]."""
  dt = w[MD + 'iou_token.weight'].dtype
  embedding, coords = embedding.to(dt), coords.to(dt)
  G = w[PE + 'pe_layer.positional_encoding_gaussian_matrix']
  n = coords.shape[0]
  ln = lambda x, name: F.layer_norm(x, (256,), w[name + '.weight'], w[name + '.bias'], ln_eps)
  pts = pos_enc(G, (coords + 0.5) / 1024)
  pts = pts + torch.where(labels[..., None] > 0, w[PE + 'point_embeddings.1.weight'], w[PE + 'point_embeddings.0.weight'])
  tok_pe = torch.cat([w[MD + 'iou_token.weight'].expand(n, 1, 256), w[MD + 'mask_tokens.weight'].expand(n, 4, 256), pts,
                      w[PE + 'not_a_point_embed.weight'].expand(n, 1, 256)], 1)
  ax = (torch.arange(64, dtype=dt) + 0.5) / 64
  pos = pos_enc(G, torch.stack(torch.meshgrid(ax, ax, indexing='xy'), -1)).reshape(1, 4096, 256)      # [i, j] -> (x_j, y_i)
  k = (embedding.reshape(256, 4096).T + w[PE + 'no_mask_embed.weight']).expand(n, 4096, 256)
  q = tok_pe
  for i in range(2):
    L = f'{TR}layers.{i}.'
    if i == 0:
      q = _attn(w, L + 'self_attn', q, q, q)
    else:
      q = q + _attn(w, L + 'self_attn', q + tok_pe, q + tok_pe, q)
    q = ln(q, L + 'norm1')
    q = ln(q + _attn(w, L + 'cross_attn_token_to_image', q + tok_pe, k + pos, k), L + 'norm2')
    h = F.relu(F.linear(q, w[L + 'mlp.lin1.weight'], w[L + 'mlp.lin1.bias']))
    q = ln(q + F.linear(h, w[L + 'mlp.lin2.weight'], w[L + 'mlp.lin2.bias']), L + 'norm3')
    k = ln(k + _attn(w, L + 'cross_attn_image_to_token', k + pos, q + tok_pe, q), L + 'norm4')
  q = ln(q + _attn(w, TR + 'final_attn_token_to_image', q + tok_pe, k + pos, k), TR + 'norm_final_attn')
  up = F.conv_transpose2d(k.transpose(1, 2).reshape(n, 256, 64, 64), w[MD + 'output_upscaling.0.weight'],
                          w[MD + 'output_upscaling.0.bias'], stride=2)
  up = F.layer_norm(up.permute(0, 2, 3, 1), (64,), w[MD + 'output_upscaling.1.weight'], w[MD + 'output_upscaling.1.bias'], 1e-6)
  up = F.gelu(F.conv_transpose2d(F.gelu(up).permute(0, 3, 1, 2), w[MD + 'output_upscaling.3.weight'],
                                 w[MD + 'output_upscaling.3.bias'], stride=2))
  hyper = torch.stack([_mlp3(w, f'{MD}output_hypernetworks_mlps.{m}', q[:, 1 + m]) for m in range(4)], 1)
  masks = (hyper @ up.flatten(2)).reshape(n, 4, 256, 256)
  return masks[:, 1:], _mlp3(w, MD + 'iou_prediction_head', q[:, 0])[:, 1:]


def input_size(h, w):
  s = 1024 / max(h, w)
  return int(h * s + 0.5), int(w * s + 0.5)


def postprocess(lowres, in_size, size):
  """segment_anything's postprocess_masks: [N,C,256,256] -> [N,C,H,W]."""
  x = F.interpolate(lowres, (1024, 1024), mode='bilinear', align_corners=False)[..., :in_size[0], :in_size[1]]
  return F.interpolate(x, size, mode='bilinear', align_corners=False)
