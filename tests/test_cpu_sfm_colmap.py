"""The COLMAP readers behind nerf_hugs_amd.hugs.sfm_prompts_from_colmap (internal/colmap.py: read_images_points2D,
read_points3D_track_lengths) and the host-side assembly of one image's (xys, track_len): a three-image, six-point sparse model
written with struct.pack, read back."""
import struct

import numpy as np

# image id -> (name, camera id, [(x, y, point3D_id)]); point3D id -> track length.  Ids are not contiguous and not in file order.
IMAGES = {7: ('images/a_000.png', 2, [(10.5, 20.25, 11), (700.125, -3.5, -1), (333.0, 444.0, 40), (12.0, 500.75, 12)]),
          3: ('b_001.jpg', 1, []),
          9: ('c_002.png', 2, [(1.0, 2.0, 13), (3.0, 4.0, -1), (5.0, 6.0, 14), (7.0, 8.0, 11), (9.0, 10.0, 15)])}
TRACKS = {11: 6, 12: 2, 13: 5, 14: 1, 15: 9, 40: 3}
CAMERAS = {1: (1, 800, 600, (500., 500., 400., 300.)), 2: (2, 1297, 840, (900., 648.5, 420., 0.01))}


def write_model(path):
  with open(path / 'cameras.bin', 'wb') as f:
    f.write(struct.pack('<Q', len(CAMERAS)))
    for cid, (model, w, h, params) in CAMERAS.items():
      f.write(struct.pack('<iiQQ', cid, model, w, h) + struct.pack(f'<{len(params)}d', *params))
  with open(path / 'images.bin', 'wb') as f:
    f.write(struct.pack('<Q', len(IMAGES)))
    for iid, (name, cid, obs) in IMAGES.items():
      f.write(struct.pack('<i7di', iid, 1., 0., 0., 0., .1, .2, .3, cid) + name.encode() + b'\0' + struct.pack('<Q', len(obs)))
      for x, y, pid in obs:
        f.write(struct.pack('<ddq', x, y, pid))
  with open(path / 'points3D.bin', 'wb') as f:
    f.write(struct.pack('<Q', len(TRACKS)))
    for pid, tl in TRACKS.items():
      f.write(struct.pack('<Q3d3BdQ', pid, 1., 2., 3., 4, 5, 6, .5, tl) + b''.join(struct.pack('<ii', t, t) for t in range(tl)))
  return path


def test_readers_and_observations(tmp_path):
  from nerf_hugs_amd import hugs
  from nerf_hugs_amd.internal import colmap
  write_model(tmp_path)
  imgs = colmap.read_images_points2D(str(tmp_path / 'images.bin'))
  assert list(imgs) == list(IMAGES)
  for iid, (name, cid, obs) in IMAGES.items():
    got = imgs[iid]
    assert got[:2] == (name, cid)
    assert got[2].dtype == np.float64 and got[2].shape == (len(obs), 2) and got[3].dtype == np.int64
    assert np.array_equal(got[2], np.array([o[:2] for o in obs], np.float64).reshape(-1, 2)) and got[3].tolist() == [o[2] for o in obs]
  assert colmap.read_points3D_track_lengths(str(tmp_path / 'points3D.bin')) == TRACKS
  # the readers that were there before see the same file
  assert {k: v['name'] for k, v in colmap.read_images_binary(str(tmp_path / 'images.bin')).items()} == {k: v[0] for k, v in IMAGES.items()}
  assert colmap.read_points3D_binary(str(tmp_path / 'points3D.bin')).shape == (6, 3)
  for model in (str(tmp_path), hugs.read_sfm_model(str(tmp_path))):
    xys, track_len, cam = hugs.sfm_observations(model, 'a_000')      # by stem, directories and extension dropped (:212)
    assert np.array_equal(xys, np.array([o[:2] for o in IMAGES[7][2]])) and xys.dtype == np.float64
    assert track_len.dtype == np.int32 and track_len.tolist() == [6, -1, 3, 2] and cam == (840, 1297)
  xys, track_len, cam = hugs.sfm_observations(str(tmp_path), 'b_001')
  assert xys.shape == (0, 2) and track_len.shape == (0,) and cam == (600, 800)
