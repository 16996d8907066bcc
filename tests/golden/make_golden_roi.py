"""Generate ``tests/golden/G12_roi.npz`` by running the reference's ``WUtils.Simulator.get_roi_signals`` on CPU.

Run once in the build container (the GPU box has no /root/reference):

    python tests/golden/make_golden_roi.py

The reference (``/root/reference``, read-only) is imported as it is, the way ``make_golden.py`` imports it.  Only data is
written: a seeded 20 x 16 x 2 x 5 video of positive values (no NaN: the reference smears a NaN over its whole box through
the spline prefilter of ``affine_transform``, which the product does not reproduce), K = 6 tracks and the reference's
signals for the windows [3, 3, 0] and [2, 1, 1].  The tracks: one within the window of every low face, one within it of
every high face, one exactly on the last voxel, two at ``.5`` coordinates (``torch.round`` rounds half to even), one that
moves through the interior.  Before writing, the numpy restatement of the tests (``tests/tracks_restatement.py``) is checked
against the reference under the tolerance the tests use (N 2^-23 relative, N the voxels of the box: the reference sums the
box in float32)."""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
WINDOWS = ([3, 3, 0], [2, 1, 1])


def tracks(T):
    t = np.arange(T, dtype=np.float32)
    base = np.array([[1.2, 0.7, 0.2], [18.4, 14.6, 0.8], [19.0, 15.0, 1.0], [6.5, 7.5, 0.5], [10.0, 8.0, 0.3], [2.5, 12.5, 1.0]],
                    dtype=np.float32)
    step = np.array([[0.4, 0.3, 0.0], [-0.3, -0.2, 0.0], [0.0, 0.0, 0.0], [1.0, -1.0, 0.0], [0.7, -0.6, 0.1], [1.0, 0.0, 0.0]],
                    dtype=np.float32)
    return torch.from_numpy(base[:, :, None] + step[:, :, None] * t[None, None, :])


def main():
    sys.path.insert(0, REF)
    from WUtils import Simulator
    sys.path.insert(0, os.path.join(os.path.dirname(OUT)))
    import tracks_restatement as TR
    torch.manual_seed(12)
    video = torch.rand(20, 16, 2, 5) + 0.05
    P = tracks(5)
    out = {"video": video.numpy(), "P": P.numpy()}
    for i, w in enumerate(WINDOWS):
        sig = Simulator.get_roi_signals(video, P, np.array(w))
        mine = TR.roi_signals(video.numpy(), P.numpy(), w)
        n = int(np.prod([2 * v + 1 for v in w]))
        err = np.abs(mine - sig).max() / np.abs(sig).min()
        print(f"window {w}: restatement vs reference, max relative error {err:.3e}, bound {n * 2.0 ** -23:.3e}")
        np.testing.assert_allclose(mine, sig, rtol=n * 2.0 ** -23, atol=0)
        out[f"window{i}"], out[f"signals{i}"] = np.array(w), sig
    path = os.path.join(OUT, "G12_roi.npz")
    np.savez_compressed(path, **out)
    print(f"G12_roi: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
