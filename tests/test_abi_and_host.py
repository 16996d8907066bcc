"""CPU-side checks of the product: the C-ABI library loads and exports every symbol the header declares,
argument validation works without a GPU, and the host-side simulator reproduces the reference video."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden


@pytest.fixture(scope="module")
def lib():
    from dnmf_amd.build import build_library
    build_library()
    from dnmf_amd import _lib
    return _lib.load()


def header_functions():
    text = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    from dnmf_amd import _lib
    names = header_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dnmf_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype in dnmf_amd/_lib.py"
    assert sorted(_lib.SIGNATURES) == names


_CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
          "float": ctypes.c_float, "dnmf_stream_t": ctypes.c_void_p, "dnmf_comm_t": ctypes.c_void_p}


def header_prototypes():
    """{name: (restype, [argtypes])} of every dnmf_* prototype of include/dnmf_hip.h, as ctypes: comments and preprocessor
    lines stripped, any pointer (and the two handle typedefs) a c_void_p, a ``const char *`` result a c_char_p."""
    text = open(os.path.join(ROOT, "include", "dnmf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)

    def ctype(decl, name):
        if "*" in decl:
            return ctypes.c_void_p
        words = [w for w in decl.split() if w != "const"]
        if words[-1] not in _CTYPE:      # a parameter name follows the type
            words.pop()
        assert len(words) == 1 and words[0] in _CTYPE, f"{name}: type of '{decl}'"
        return _CTYPE[words[0]]

    out = {}
    for res, name, args in re.findall(r"([A-Za-z_][\w \t]*?[\s*]+)(dnmf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        args = " ".join(args.split())
        restype = ctypes.c_char_p if re.fullmatch(r"const\s+char\s*\*\s*", res) else ctype(res, name)
        assert name not in out, f"{name} declared twice"
        out[name] = (restype, [] if args in ("", "void") else [ctype(a, name) for a in args.split(",")])
    return out


def test_every_prototype_equals_its_ctypes_signature(lib):
    """The binding whole: result type and argument list of every function the header declares against
    ``_lib.SIGNATURES``, and one ABI version in the header, the binding and the library as built."""
    from dnmf_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_functions() == sorted(_lib.SIGNATURES) and len(protos) >= 96
    for name, proto in protos.items():
        assert proto == _lib.SIGNATURES[name], f"{name}: header {proto} != SIGNATURES {_lib.SIGNATURES[name]}"
    version = re.search(r"^#define\s+DNMF_ABI_VERSION\s+(\d+)\s*$", open(os.path.join(ROOT, "include", "dnmf_hip.h")).read(), re.M)
    assert int(version.group(1)) == _lib.ABI_VERSION == lib.dnmf_version()


def test_kernel_forms_are_arguments_not_environment(lib, monkeypatch):
    """The launch form of K3n and the axis kernel of K8 are arguments.  (0, 0) is the library's choice: the table counts a
    build with the former four-argument dnmf_warp_gram_rhs_lists_chunks returned; passes 1 | 2 times chunks 1 | 3 gives
    passes x chunks tables while the chunks fit the tiles (3 at 24 x 20, 1024 at 512 x 512); the environment variables
    that once chose the forms change nothing; values outside passes 0..2, chunks 0..64, valu 0..1 are refused before any
    HIP call."""
    shapes = (((24, 20, 1, 4), 3, 3), ((512, 512, 1, 4000), 10, 1024))

    def counts():
        got = [lib.dnmf_warp_gram_rhs_lists_chunks(*shape, 0, 0) for shape, _, _ in shapes]
        return got + [lib.dnmf_warp_gram_rhs_lists_chunks(*shape, p, c) for shape, _, _ in shapes for p in (1, 2) for c in (1, 3)]

    expected = [auto for _, auto, _ in shapes] + [p * min(c, ntiles) for _, _, ntiles in shapes for p in (1, 2) for c in (1, 3)]
    assert counts() == expected
    assert lib.dnmf_warp_gram_rhs_lists_chunks(8, 32, 1, 4, 2, 3) == 2 * 1         # one tile: the request is clipped to it
    assert lib.dnmf_warp_gram_rhs_lists_chunks(512, 512, 1, 4000, 0, 64) == 10     # above what the workspace holds: the choice
    for name, value in (("DNMF_LISTS_PASSES", "1"), ("DNMF_LISTS_CHUNKS", "3"), ("DNMF_K8_VALU", "1")):
        monkeypatch.setenv(name, value)
    assert counts() == expected
    for passes, chunks in ((3, 0), (-1, 0), (0, 65), (0, -1)):
        assert lib.dnmf_warp_gram_rhs_lists_chunks(512, 512, 1, 4000, passes, chunks) == 0
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    I3 = ctypes.c_int * 3
    gram = lambda passes, chunks: lib.dnmf_warp_gram_rhs_lists(a, a, a, a, 10, 3, 4, 4, 1, a, 1, None, 1, a, 16, None, a, a, a,
                                                               1 << 20, None, passes, chunks, None)
    for passes, chunks in ((3, 0), (0, 65)):
        assert gram(passes, chunks) == -2 and b"passes=" in lib.dnmf_last_error()
    patches = lambda valu: lib.dnmf_register_patches(a, 20 * 20, None, 1, a, 20, 20, 1, I3(8, 8, 1), I3(4, 4, 0), I3(0, 12, 0), 3,
                                                     10, 0.0, a, a, a, 64, valu, None)
    rigid = lambda valu: lib.dnmf_rigid_correct(a, 20 * 20, None, 1, a, 20, 20, 1, I3(0, 12, 0), 10, 0.0, 1, a, None, 0, None,
                                                None, a, 64, valu, None)
    for call in (patches, rigid):
        assert call(2) == -2 and b"valu=2" in lib.dnmf_last_error()
        assert call(0) == call(1) == -4       # both kernels go on to the workspace check


def test_version_and_padding(lib):
    assert lib.dnmf_version() == 7
    assert [lib.dnmf_padded_k(k) for k in (0, 1, 10, 15, 16, 50, 100, 111, 112, 200)] == \
        [0, 16, 16, 16, 32, 64, 112, 112, 128, 208]


def test_argument_errors_are_reported_without_a_gpu(lib):
    """Validation happens before any HIP call, so it can be exercised on a CPU-only box."""
    rc = lib.dnmf_pack_footprints(None, 10, 3, None, 16, None)
    assert rc == -1 and b"NULL" in lib.dnmf_last_error()
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    rc = lib.dnmf_pack_footprints(addr, 10, 3, addr, 17, None)
    assert rc == -2 and b"Kp" in lib.dnmf_last_error()
    rc = lib.dnmf_mu_temporal(addr, addr, addr, 4, 300, 4, 1, None)
    assert rc == -3
    rc = lib.dnmf_warp_gram_rhs(addr, 16, 3, 0, 4, 4, 1, addr, 1, None, 1, addr, 16, None, addr, addr, addr, 8, None)
    assert rc in (-2, -4)  # alignment or workspace, never a launch
    assert lib.dnmf_warp_gram_rhs_workspace(262144, 100, 4000) == 4000 * 3 * 28 * 256 * 4
    # the neuron-list entry points
    assert lib.dnmf_pack_footprints_lists(addr, 4, 4, 1, 300, addr, addr, addr, addr, addr, None) == -3   # K > 256
    assert lib.dnmf_pack_footprints_lists(None, 4, 4, 1, 3, addr, addr, addr, addr, addr, None) == -1
    assert lib.dnmf_halo_row(512, 1) == 544 and lib.dnmf_halo_row(5, 3) == 32     # rows start on 128-byte lines
    assert lib.dnmf_halo_voxels(512, 512, 1) == 516 * 544 and lib.dnmf_halo_voxels(4, 5, 3) == 8 * 32
    assert lib.dnmf_lists_axis_masks_bytes(512, 512, 1, 100) == 2 * (512 + 512 + 1 + 6) * 2 * 8
    # slot tables (5 chunks per frame at B = 4000, two tables per chunk: one per launch; rounded up to 256 bytes), then one
    # 2-word list and one 16-byte descriptor per frame and tile
    slab = (4000 * 2 * 5 * 461 * 4 + 255) // 256 * 256
    assert lib.dnmf_warp_gram_rhs_lists_chunks(512, 512, 1, 4000, 0, 0) == 10     # tables a consumer sums per frame
    assert lib.dnmf_warp_gram_rhs_lists_chunks(512, 512, 1, 400, 0, 0) == 41      # short video: one launch, one table per chunk
    assert lib.dnmf_warp_gram_rhs_lists_workspace(461, 100, 512, 512, 1, 4000) == slab + 4000 * 1024 * (2 * 8 + 16)
    rc = lib.dnmf_warp_gram_rhs_lists(addr, addr, addr, addr, 5000, 3, 4, 4, 1, addr, 1, None, 1, addr, 16, None, addr, addr,
                                      addr, 1 << 20, None, 0, 0, None)
    assert rc == -3 and b"pattern slots" in lib.dnmf_last_error()
    rc = lib.dnmf_warp_gram_rhs_lists(addr, addr, addr, addr, 10, 3, 4, 4, 1, addr, 1, None, 1, addr, 16, None, addr, addr,
                                      addr, 8, None, 0, 0, None)
    assert rc == -4
    assert lib.dnmf_recon_image_lists(addr, addr, 3, 4, 4, 1, addr, 4, None, 2, addr, 16, None) == -2    # lds < 8 x 32
    assert lib.dnmf_mu_temporal_nbr(addr, addr, addr, 4, 3, 4, 1, addr, 12, None) == -3                   # NN not 8/16/32
    assert lib.dnmf_adam_epoch_workspace(1000) == 16000
    assert lib.dnmf_adam_epoch(addr, None, addr, addr, 4, 0, addr, None, 10, 1e-3, 0.9, 0.999, 1e-8, 0, addr, 8, None) == -4
    assert lib.dnmf_warp_recon_grad_workspace(512, 512, 1, 4000) == 512 * 8 + 4000 * 32 * 32 * 4 + 4000 * 4
    # K2 at Z == 2 reads a column's two slices as one aligned pair: an odd frame stride is refused (lds = 8 x 32, P = 32)
    k2 = lambda ldf, ws: lib.dnmf_warp_recon_grad(addr, 256, None, addr, ldf, None, None, 4, 4, 2, addr, 1, addr, 1, 0, None, addr,
                                                  None, None, None, addr, ws, None)
    assert k2(33, 1 << 20) == -2 and b"even ldf" in lib.dnmf_last_error()
    assert k2(34, 8) == -4                                            # an even one goes on to the workspace check
    assert lib.dnmf_warp_recon_grad(addr, 256, None, addr, 17, None, None, 4, 4, 1, addr, 1, addr, 1, 0, None, addr, None, None,
                                    None, addr, 8, None) == -4        # Z == 1: any stride
    mg = lambda ldf: lib.dnmf_motion_grad_lists(addr, addr, 3, addr, 1, addr, ldf, None, 4, 4, 2, addr, 1, addr, 1, 1, addr, None,
                                                None, 1, addr, 8, None)
    assert mg(33) == -2 and b"even ldf" in lib.dnmf_last_error()
    assert mg(34) == -4
    # C1: arguments are checked before RCCL is looked up
    assert lib.dnmf_comm_unique_id(None) == -1
    assert lib.dnmf_comm_init(None, addr, 2, 0) == -1
    handle = ctypes.c_void_p()
    assert lib.dnmf_comm_init(ctypes.byref(handle), addr, 2, 2) == -2 and b"rank 2 of 2" in lib.dnmf_last_error()
    assert lib.dnmf_allreduce_sum_f32(None, addr, 4, None) == -1
    assert lib.dnmf_comm_destroy(None) == 0


def test_gram_workspace_values(lib):
    """What the workspace functions of K3 / K3b and of both K3s variants return, pinned: B * (max chunks + 1) work-item
    regions, max chunks = min(64, ceil(target / B)) with target 4096 (K3) or 8192 (K3s); a K3 item holds the NT =
    NB(NB+1)/2 upper-triangle tiles of 256 floats, a K3s item NT tiles (static) or the NB x NB grid (table) plus 128
    floats of right-hand side."""
    assert lib.dnmf_warp_gram_rhs_workspace(262144, 100, 4000) == 4000 * 3 * 28 * 256 * 4
    assert lib.dnmf_warp_gram_rhs_workspace(262144, 100, 1) == 65 * 28 * 256 * 4
    for (P, K, B), static, table in (((262144, 100, 4000), 466944000, 811008000), ((262144, 100, 1), 1896960, 3294720),
                                     ((1024, 16, 100), 9984000, 9984000)):
        NB = (K + 15) // 16
        chunks = min(64, -(-8192 // B)) + 1
        assert static == B * chunks * (NB * (NB + 1) // 2 * 256 + 128) * 4 and table == B * chunks * (NB * NB * 256 + 128) * 4
        assert lib.dnmf_warp_gram_rhs_sparse_workspace(P, K, B) == static
        assert lib.dnmf_warp_gram_rhs_sparse_lt_workspace(P, K, B) == table
    for fn in (lib.dnmf_warp_gram_rhs_workspace, lib.dnmf_warp_gram_rhs_sparse_workspace,
               lib.dnmf_warp_gram_rhs_sparse_lt_workspace):
        for args in ((0, 100, 4), (-1, 100, 4), (1024, 0, 4), (1024, -3, 4), (1024, 100, 0), (1024, 100, -1)):
            assert fn(*args) == 0, (fn, args)


def test_product_has_no_cpu_fallback():
    """The classes need the HIP library and a GPU; on a CPU box construction raises instead of computing."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dnmf_amd.Demix import dNMF
    with pytest.raises(Exception):
        dNMF.ExponentialFP(torch.tensor([8, 8, 2]), 2, 3, positions=torch.zeros(2, 3))
    import dnmf_amd
    src = "".join(open(os.path.join(os.path.dirname(dnmf_amd.__file__), f)).read()
                  for f in ("ops.py", "_lib.py", os.path.join("Demix", "dNMF.py")))
    assert "oracle" not in src.replace("CPU oracle", "")


def chan_of(NB, b, i):
    """Python mirror of csrc/warp_gram_rhs.hip:chan_of -- the channel held by lane slot i for block b."""
    ng4, r = divmod(NB, 4)
    if b < 4 * ng4:
        return 64 * (b // 4) + 4 * i + (b % 4)
    return 64 * ng4 + r * i + (b - 4 * ng4)


@pytest.mark.parametrize("NB", range(1, 9))
def test_gram_channel_permutation_is_a_bijection(NB):
    seen = sorted(chan_of(NB, b, i) for b in range(NB) for i in range(16))
    assert seen == list(range(16 * NB))
    assert chan_of(NB, NB - 1, 15) == 16 * NB - 1   # the frame column is the last pad channel


def test_simulator_reproduces_reference_video():
    from dnmf_amd.WUtils import Simulator as S
    g = golden("G8_simulator")
    par = {"sigma": [5, 5, .01], "ls": [10, 10, 10]}
    for snr, key in ((-120, "video"), (-20, "video_noisy")):
        torch.manual_seed(0)
        np.random.seed(0)
        video, positions, traces = S.generate_video(3, 6, g["sz"], 3, .2, snr, 'exp', 'gp', par)
        np.testing.assert_allclose(video.numpy(), g[key], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(positions.numpy(), g["positions"], rtol=1e-6, atol=1e-6)
        np.testing.assert_array_equal(traces, g["traces"])
    with pytest.raises(NotImplementedError):
        S.generate_video(3, 6, [8, 8, 2], motion='sq')


def test_dataset_protocol_and_in_place_clamp():
    from dnmf_amd.Demix.dNMF import SimulatedVideoDataset
    torch.manual_seed(0)
    np.random.seed(0)
    ds = SimulatedVideoDataset(K=3, T=6, sz=torch.tensor([16, 16, 2]), shape_std=3, density=.2, bg_snr=-20,
                               traces='exp', motion='gp', motion_par={"sigma": [5, 5, .01], "ls": [10, 10, 10]})
    assert len(ds) == 6 and tuple(ds.video.shape) == (16, 16, 2, 6) and tuple(ds.positions.shape) == (3, 3, 6)
    assert float(ds.video.min()) < 0
    frame, idx = ds[2]
    assert idx == 2 and float(frame.min()) >= 0 and float(ds.video[..., 2].min()) >= 0   # clamped in the store
    assert float(ds.video[..., 3].min()) < 0
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)
    batch = next(iter(loader))
    assert tuple(batch[0].shape) == (4, 16, 16, 2) and batch[1].tolist() == [0, 1, 2, 3]


def test_index_batches_of_a_stock_dataloader_without_fetching_samples():
    """``DeformableNMF._resident_batches``: for a dataset that hands over its frames (``device_frames()``) only the index
    batches of a stock DataLoader are drawn -- the same batches, and the same draws from the global generator, as an
    ordinary pass over the loader; other loaders are left alone."""
    from dnmf_amd.Demix.dNMF import DeformableNMF

    class Frames(torch.utils.data.Dataset):
        fetched = 0

        def __init__(self, n, row):
            self.frames = torch.arange(n * row, dtype=torch.float32).reshape(n, row)

        def device_frames(self):
            return self.frames

        def __len__(self):
            return self.frames.shape[0]

        def __getitem__(self, i):
            Frames.fetched += 1
            return self.frames[i], i

    ds = Frames(11, 6)
    for shuffle in (False, True):
        torch.manual_seed(5)
        ordinary = [idx.tolist() for _, idx in torch.utils.data.DataLoader(ds, batch_size=4, shuffle=shuffle)]
        after_ordinary = float(torch.rand(1))
        Frames.fetched = 0
        torch.manual_seed(5)
        frames, batches = DeformableNMF._resident_batches(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=shuffle), 6)
        assert batches == ordinary and Frames.fetched == 0 and frames is ds.frames
        assert float(torch.rand(1)) == after_ordinary
    assert [len(b) for b in batches] == [4, 4, 3]
    dropped = DeformableNMF._resident_batches(torch.utils.data.DataLoader(ds, batch_size=4, drop_last=True), 6)[1]
    assert [len(b) for b in dropped] == [4, 4]
    # not taken: a row length the model does not expect, a custom collate function, a dataset without device_frames
    assert DeformableNMF._resident_batches(torch.utils.data.DataLoader(ds, batch_size=4), 7) is None
    assert DeformableNMF._resident_batches(torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=lambda b: b), 6) is None
    plain = torch.utils.data.TensorDataset(ds.frames, torch.arange(11))
    assert DeformableNMF._resident_batches(torch.utils.data.DataLoader(plain, batch_size=4), 6) is None
    assert DeformableNMF._resident_batches([(ds.frames[:4], torch.arange(4))], 6) is None


def test_neuropal_dataset_reads_mat_files(tmp_path):
    """The real-data loader of the reference (its data is not in the tree): round trip through scipy's .mat files."""
    from scipy.io import savemat
    from dnmf_amd.Demix.dNMF import NeuroPALVideoDataset
    rng = np.random.RandomState(0)
    data = rng.randn(12, 10, 20, 5)
    pos = 1 + rng.rand(4, 3, 5) * np.array([12, 10, 20])[None, :, None]
    savemat(tmp_path / "data.mat", {"data": data})
    savemat(tmp_path / "traces_n.mat", {"positions": pos, "neuron_names": np.array([["a", "b", "c", "d"]], dtype=object)})
    ds = NeuroPALVideoDataset(str(tmp_path))
    assert len(ds) == 5 and ds.video.shape == (6, 5, 2, 5) and tuple(ds.positions.shape) == (4, 3, 5)
    np.testing.assert_allclose(ds.positions[:, 0].numpy(), (pos[:, 0] - 1) / 2, rtol=1e-6)
    np.testing.assert_allclose(ds.positions[:, 2].numpy(), (pos[:, 2] - 1) / 10, rtol=1e-6)
    frame, idx = ds[3]
    assert idx == 3 and frame.min() >= 0 and frame.shape == (6, 5, 2)


def test_patch_grid_and_workspaces_of_the_position_initialiser(lib):
    """K8's host logic without a GPU: the patch grid equals the oracle's sliding_window_3d (reference
    MotionCorrect.py:1190-1221) -- windows of strides + overlaps every `strides`, the last one flush with the end --, windows
    that do not fit are refused, and the workspaces grow with the number of frames."""
    from oracle import motion_oracle as MO
    I3 = ctypes.c_int * 3
    for sz, strides, overlaps in (((48, 40, 2), (16, 12, 1), (8, 8, 1)), ((512, 512, 2), (96, 96, 1), (32, 32, 1)),
                                  ((40, 36, 5), (12, 12, 2), (8, 6, 1)), ((64, 64, 1), (24, 24, 1), (8, 8, 0))):
        ref = MO.sliding_window_3d(sz, overlaps, strides)
        dims = I3()
        NP = lib.dnmf_register_patches_grid(*sz, I3(*strides), I3(*overlaps), dims, None)
        assert NP == len(ref) and tuple(dims) == tuple(np.array(ref[-1][:3]) + 1)
        starts = (ctypes.c_int * (3 * NP))()
        assert lib.dnmf_register_patches_grid(*sz, I3(*strides), I3(*overlaps), dims, starts) == NP
        np.testing.assert_array_equal(np.array(starts).reshape(NP, 3), np.array([g[3:6] for g in ref]))
        w1 = lib.dnmf_register_patches_workspace(*sz, I3(*strides), I3(*overlaps), 1)
        w8 = lib.dnmf_register_patches_workspace(*sz, I3(*strides), I3(*overlaps), 8)
        assert 0 < w1 <= w8
        assert 0 < lib.dnmf_rigid_correct_workspace(*sz, 1) <= lib.dnmf_rigid_correct_workspace(*sz, 8)
    assert lib.dnmf_register_patches_grid(32, 32, 2, I3(24, 24, 1), I3(16, 16, 1), None, None) == 0      # 40 > 32: no window fits
    assert lib.dnmf_register_patches_workspace(32, 32, 2, I3(24, 24, 1), I3(16, 16, 1), 4) == 0
    assert lib.dnmf_rigid_correct_workspace(0, 4, 4, 1) == 0


def _r256(b):
    return (b + 255) // 256 * 256


def k8_pass_needs(boxes, uf=10):
    """float2 values each buffer of one K8 registration receives, from the launch shapes of McRun (register_patches.hip): an
    axis pass writes McAxis.out = (items, outer, m, inner).  boxes: [(items, (n0, n1, n2))].  The forward transform writes
    items n0 n1 n2 three times (spectra, ping-pong); the windowed inverse, with mm = 32 kept indices per axis (unused window
    slots are written as zeros), writes (items, 1, mm, n1 n2) to inv1, (items, mm, mm, n2) to inv2 and (items, mm mm, mm, 1)
    to cc; the upsampled inverse the same with mm = ceil(1.5 uf) <= 32.  inv2 is held to mm max(n1, mm) n2."""
    need = {"spec": 0, "inv1": 0, "inv2": 0, "cc": 0}
    region = (3 * uf + 1) // 2
    for items, (n0, n1, n2) in boxes:
        for mm in (32, region):
            need["spec"] = max(need["spec"], items * n0 * n1 * n2)
            need["inv1"] = max(need["inv1"], items * mm * n1 * n2)
            need["inv2"] = max(need["inv2"], items * mm * max(n1, mm) * n2)
            need["cc"] = max(need["cc"], items * mm ** 3)
    return need


# (size, strides, overlaps): boxes whose second axis is shorter than the 32 kept window indices, the existing geometries, and
# the size the README gives for the initialiser
K8_GEOMETRIES = (
    ((64, 16, 4), None, None), ((20, 20, 1), (8, 8, 1), (4, 4, 0)), ((40, 8, 16), None, None),
    ((36, 20, 8), (12, 6, 4), (6, 4, 4)), ((40, 20, 3), (28, 12, 2), (12, 8, 1)),
    ((48, 40, 2), (16, 12, 1), (8, 8, 1)), ((40, 36, 5), (12, 12, 2), (8, 6, 1)), ((64, 64, 1), (24, 24, 1), (8, 8, 0)),
    ((72, 50, 3), (20, 14, 2), (10, 8, 1)), ((64, 56, 1), (24, 20, 1), (8, 8, 0)), ((64, 64, 2), (16, 16, 1), (16, 16, 1)),
    ((512, 512, 2), (24, 24, 1), (8, 8, 1)), ((512, 512, 2), (96, 96, 1), (32, 32, 1)),
)


@pytest.mark.parametrize("sz,strides,overlaps", K8_GEOMETRIES)
def test_position_initialiser_workspace_holds_what_its_passes_write(lib, sz, strides, overlaps):
    """The workspaces of dnmf_register_patches / dnmf_rigid_correct against a model of what every pass writes (one frame, so
    one frame per chunk whatever the chunk policy): at least the sum of the 256-byte-rounded needs -- a box whose second
    axis is shorter than 32 writes (items, 32, 32, n2) partial inverses, more than (items, 32, n1, n2) -- and not much
    more, so that the partial inverses are not sized for the whole volume times every patch."""
    I3 = ctypes.c_int * 3
    X, Y, Z = sz
    P = X * Y * Z
    nmax = max(sz)
    f2, i4 = 8, 4
    if strides is None:       # a rigid-only geometry: the volume is its own single patch
        strides, overlaps = (X, Y, Z), (0, 0, 0)
    NP = lib.dnmf_register_patches_grid(X, Y, Z, I3(*strides), I3(*overlaps), None, None)
    assert NP > 0
    w = tuple(s + o for s, o in zip(strides, overlaps))
    full = k8_pass_needs([(1, (X, Y, Z))])
    both = k8_pass_needs([(1, (X, Y, Z)), (NP, w)])
    spec = max(P, NP * w[0] * w[1] * w[2])
    need_p = (2 * _r256(spec * f2) + _r256(P * f2) + _r256(NP * w[0] * w[1] * w[2] * f2)
              + _r256(both["inv1"] * f2) + _r256(both["inv2"] * f2) + _r256(both["cc"] * f2)
              + 2 * _r256(NP * 3 * 32 * i4) + _r256(NP * 3 * i4) + _r256(16384 * i4) + _r256((NP + 1) * 3 * i4) + _r256(64))
    need_r = (3 * _r256(full["spec"] * f2) + _r256(full["inv1"] * f2) + _r256(full["inv2"] * f2) + _r256(full["cc"] * f2)
              + 2 * _r256(3 * 32 * i4) + _r256(3 * i4) + _r256(16384 * i4) + 2 * _r256(64) + _r256(3 * nmax * i4) + _r256(4) + _r256(f2))
    for name, got, need in (("register_patches", lib.dnmf_register_patches_workspace(X, Y, Z, I3(*strides), I3(*overlaps), 1), need_p),
                            ("rigid_correct", lib.dnmf_rigid_correct_workspace(X, Y, Z, 1), need_r)):
        assert got >= need, f"{name} {sz}: workspace {got} < {need} bytes the passes write"
        assert got <= 1.25 * need + (1 << 20), f"{name} {sz}: workspace {got} bytes for {need} needed"


def test_position_initialiser_refuses_windows_it_cannot_hold(lib):
    """max_shifts = 0 zeroes nothing in the reference (numpy's cc[0:-0] is empty): the whole axis is searched, which K8
    holds only up to 32 voxels.  Refused before any HIP call."""
    I3 = ctypes.c_int * 3
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    for ms, rc in (((0, 5, 1), -3), ((5, 0, 1), -3), ((17, 5, 1), -3)):
        assert lib.dnmf_register_patches(a, 64 * 40 * 2, None, 1, a, 64, 40, 2, I3(16, 12, 1), I3(8, 8, 1), I3(*ms), 3, 10, 0.0,
                                         a, a, a, 64, 0, None) == rc, ms
        assert lib.dnmf_rigid_correct(a, 64 * 40 * 2, None, 1, a, 64, 40, 2, I3(*ms), 10, 0.0, 1, a, None, 0, None, None, a, 64,
                                      0, None) == rc, ms
    # an axis of at most 32 voxels is searched whole whatever max_shifts says; a small workspace is then the only objection
    assert lib.dnmf_register_patches(a, 20 * 20, None, 1, a, 20, 20, 1, I3(8, 8, 1), I3(4, 4, 0), I3(0, 12, 0), 3, 10, 0.0,
                                     a, a, a, 64, 0, None) == -4
    assert lib.dnmf_rigid_correct(a, 20 * 20, None, 1, a, 20, 20, 1, I3(0, 12, 0), 10, 0.0, 1, a, None, 0, None, None, a, 64,
                                  0, None) == -4


def sl_splits(X, Y, Z, T):
    """Python restatement of csrc/spatial_update.hip:sl_splits -- the frame splits of the list-form K5: enough (tile, split)
    waves to fill the GPU (>= 8192, at most 64 splits), but whole runs of 64 frames per split."""
    ntiles = (X + 3) // 4 * ((Y * Z + 63) // 64)
    s = min(max((8192 + ntiles - 1) // ntiles, 1), 64)
    while s > 1 and T // s < 64:
        s -= 1
    return s


# (X, Y, Z, T, splits, frames per split): the ragged case (a full run and a run of 3 per split, a last split of 62), exactly
# two runs, one frame short of them, the bench geometry (GPU tests: T = 600; bench: T = 4000), a volume deeper than a tile
SL_SPLIT_CASES = (
    (32, 32, 2, 1000, 15, 67), (32, 32, 2, 128, 2, 64), (32, 32, 2, 127, 1, 127), (32, 32, 2, 70, 1, 70),
    (512, 512, 1, 600, 8, 75), (512, 512, 1, 4000, 8, 500), (12, 3, 80, 300, 4, 75), (20, 16, 2, 160, 2, 80),
)


@pytest.mark.parametrize("X,Y,Z,T,ns,fps", SL_SPLIT_CASES)
def test_spatial_lists_frame_splits_and_workspace(lib, X, Y, Z, T, ns, fps):
    """The split count of the list-form K5 against its Python restatement and the counts the GPU tests
    (tests/test_gpu_spatial_lists.py) rely on; the workspace holds one compact buffer per split (none for one split); a
    workspace one float short is refused before any launch."""
    assert sl_splits(X, Y, Z, T) == ns and -(-T // ns) == fps
    assert lib.dnmf_spatial_lists_tiles(X, Y, Z) == (X + 3) // 4 * ((Y * Z + 63) // 64)
    total = 256 * 3 * lib.dnmf_spatial_lists_tiles(X, Y, Z)
    need = lib.dnmf_spatial_accum_lists_workspace(X, Y, Z, total, T)
    assert need == (ns * total * 4 if ns > 1 else 0)
    assert lib.dnmf_spatial_accum_lists_workspace(X, Y, Z, -1, T) == 0          # a list overflowed: no list form at all
    assert lib.dnmf_spatial_accum_lists_workspace(X, Y, Z, total, 0) == 0
    if ns == 1:
        return
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    P, K = X * Y * Z, 5
    for ws, nbytes in ((None, 0), (a, need - 4)):
        rc = lib.dnmf_spatial_accum_lists(a, P, None, a, T, None, T, X, Y, Z, K, a, total, a, a, ws, nbytes, None)
        assert rc == -4 and b"workspace" in lib.dnmf_last_error()
    # and the shape checks come first
    assert lib.dnmf_spatial_accum_lists(a, P - 1, None, a, T, None, T, X, Y, Z, K, a, total, a, a, None, 0, None) == -2
    assert lib.dnmf_spatial_accum_lists(None, P, None, a, T, None, T, X, Y, Z, K, a, total, a, a, None, 0, None) == -1


def test_dense_footprint_update_refusals(lib):
    """The dense K5 and K6 refuse, before any launch, what they cannot take: K5 more than 128 traces a call (the caller
    goes by column groups), rows shorter than P, frame-major traces with rows shorter than K, a NULL output; K6 more
    footprint rows than its 64 KiB of LDS hold (K = 1024 is the last it takes) and no voxels."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    P, T = 70, 21

    def k5(Y=a, ldy=P, C=a, Ct=None, ldct=0, K=20, A1=a, Cs=a, T=T):
        return lib.dnmf_spatial_accum(Y, ldy, None, C, T, Ct, ldct, None, T, P, K, A1, Cs, 0, None)

    assert k5(K=129) == -3 and b"K=129" in lib.dnmf_last_error()
    assert k5(ldy=P - 1) == -2 and b"ldy=69" in lib.dnmf_last_error()
    assert k5(Ct=a, ldct=19) == -2 and b"ldct=19" in lib.dnmf_last_error()
    assert k5(A1=None) == -1 and b"NULL" in lib.dnmf_last_error()
    assert k5(Y=None) == -1 and k5(C=None) == -1 and k5(Cs=None) == -1 and k5(T=0) == -2
    assert lib.dnmf_mu_spatial(a, a, a, None, 0.0, 17, 1025, None) == -3 and b"K=1025" in lib.dnmf_last_error()
    assert lib.dnmf_mu_spatial(a, a, a, None, 0.0, 0, 20, None) == -2 and b"P=0" in lib.dnmf_last_error()
    assert lib.dnmf_mu_spatial(None, a, a, None, 0.0, 17, 20, None) == -1
