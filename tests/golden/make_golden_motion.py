"""Generate the piecewise-rigid fixtures ``tests/golden/G11_pwrigid_*.npz`` by running the reference's
``Demix/MotionCorrect.py`` on CPU.

It needs a Python with scikit-image and scipy (the reference's 3-D piecewise path warps with ``skimage.transform``);
numpy < 2 with ``past`` (``future``) installed.  cv2 is not needed, see below.  Run it in the build container as

    <python with skimage> tests/golden/make_golden_motion.py

The reference module is imported as it is, from its file, through ``importlib``, with three accommodations that leave
its files untouched:
  * a package stub ``Demix`` so that its relative self-import (``from .MotionCorrect import *``) resolves;
  * a stub ``cv2`` module: the module imports ``idft`` / ``dft`` from cv2 and reads ``cv2.BORDER_REFLECT`` as a default
    argument (``:387``), but the 3-D piecewise path with ``shifts_opencv=True`` never calls cv2 -- every stub function
    raises if it is called, so a fixture can not silently depend on one;
  * ``np.int`` (gone from numpy 1.24) is set to ``int`` if missing, and ``pylab`` is stubbed if matplotlib is absent.

Each fixture holds data only: the input video (T, X, Y, Z) and template, the parameters, the reference's
``x/y/z_shifts_els`` (T, NP), its corrected movie ``mc`` (X, Y, Z, T) float32, its chunk template (the nanmean of the
corrected frames, ``templates_els[0]``) and its ``total_template`` -- recorded to document that ``np.dstack`` collapses a
3-D template to (X, Y) (``motion_correct_batch_pwrigid`` ``:1970``).  The .npz files are written with fixed zip
timestamps, so a second run regenerates them bit for bit.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

REF = "/root/reference/Demix/MotionCorrect.py"
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    try:
        import scipy.ndimage  # noqa: F401
        import skimage.transform  # noqa: F401
        import past.utils  # noqa: F401
    except ImportError as e:
        sys.exit(f"make_golden_motion.py needs scikit-image, scipy and past (future) in this interpreter: {e}")
    if not hasattr(np, "int"):
        np.int = int
    if "cv2" not in sys.modules:
        cv2 = types.ModuleType("cv2")
        cv2.BORDER_REFLECT = 2

        def _absent(name):
            def f(*a, **k):
                raise RuntimeError(f"cv2.{name} called: the fixture would depend on OpenCV")
            return f
        for name in ("idft", "dft", "warpAffine", "remap", "resize", "filter2D", "getGaussianKernel", "imshow", "waitKey",
                     "destroyAllWindows", "setNumThreads"):
            setattr(cv2, name, _absent(name))
        sys.modules["cv2"] = cv2
    try:
        import pylab  # noqa: F401
    except ImportError:
        sys.modules["pylab"] = types.ModuleType("pylab")
    pkg = types.ModuleType("Demix")
    pkg.__path__ = [os.path.dirname(REF)]
    sys.modules["Demix"] = pkg
    spec = importlib.util.spec_from_file_location("Demix.MotionCorrect", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["Demix.MotionCorrect"] = mod
    spec.loader.exec_module(mod)
    return mod


def blob_video(sz, T, K, seed, amp):
    """Gaussian blobs on a dim background; frame t = the template moved by a smooth, piecewise different displacement (one
    shift per quadrant of the (x, y) plane, blended by the blob position) of up to ~amp + 1 voxels in x, y and a fraction
    of a slice in z, plus a little noise (tests/test_gpu_motioncorrect.py's synthetic_video with larger shifts)."""
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    gx, gy, gz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    pos = rng.rand(K, 3) * np.array([X, Y, Z])

    def render(shift_of):
        v = np.full(sz, 0.02)
        for k in range(K):
            d = shift_of(pos[k])
            v += np.exp(-(((gx - pos[k, 0] - d[0]) / 2.5) ** 2 + ((gy - pos[k, 1] - d[1]) / 2.5) ** 2 +
                          ((gz - pos[k, 2] - d[2]) / 1.5) ** 2))
        return v

    template = render(lambda p: np.zeros(3))
    video = []
    for t in range(T):
        base = rng.uniform(-amp, amp, 3) * np.array([1, 1, 0.3 if Z > 1 else 0.0])
        quad = rng.uniform(-1.0, 1.0, (2, 2, 3)) * np.array([1, 1, 0.0])
        video.append(render(lambda p: base + quad[int(p[0] >= X / 2), int(p[1] >= Y / 2)]) + 0.002 * rng.randn(*sz))
    return np.array(video, dtype=np.float32), template.astype(np.float32)


def save(name, **arrays):
    """np.savez_compressed's layout with fixed member timestamps (bit-for-bit reproducible files)."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)
    print(f"{path}: {os.path.getsize(path)} bytes")


def make(R, name, sz, T, K, seed, amp, strides, overlaps, max_shifts, max_deviation_rigid=3):
    video, template = blob_video(sz, T, K, seed, amp)
    min_mov = float(video.min())
    add = -min_mov
    total, templates, xs, ys, zs, _, mcl = R.motion_correct_batch_pwrigid(
        video, max_shifts, strides, overlaps, add, upsample_factor_grid=4, max_deviation_rigid=max_deviation_rigid, splits=1,
        num_splits_to_process=None, num_iter=1, template=template, shifts_opencv=True, nonneg_movie=True, gSig_filt=None,
        use_cuda=False, border_nan=True, is3D=True)
    mc = np.asarray(mcl[0], dtype=np.float32)                  # (X, Y, Z, T): one chunk, every frame holds the same array
    assert mc.shape == (*sz, T) and len(templates) == 1
    save(name, video=video, template=template, min_mov=np.float64(min_mov), strides=np.array(strides),
         overlaps=np.array(overlaps), max_shifts=np.array(max_shifts), max_deviation_rigid=np.int64(max_deviation_rigid),
         x_shifts_els=np.array(xs), y_shifts_els=np.array(ys), z_shifts_els=np.array(zs), mc=mc,
         chunk_template=np.asarray(templates[0]), total_template=np.asarray(total))


def main():
    R = load_reference()
    # several patch layers in z: the n-d branch of skimage's resize
    make(R, "G11_pwrigid_3d", (32, 28, 4), 4, 14, seed=11, amp=3.0, strides=(12, 10, 2), overlaps=(6, 6, 1), max_shifts=(5, 5, 1))
    # one slice: the per-slice branch of skimage's resize (dims[2] == Z)
    make(R, "G11_pwrigid_z1", (40, 32, 1), 4, 16, seed=12, amp=3.0, strides=(14, 12, 1), overlaps=(8, 6, 0), max_shifts=(5, 5, 0))


if __name__ == "__main__":
    main()
