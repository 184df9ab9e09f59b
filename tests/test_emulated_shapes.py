"""Odd shapes through the emulated kernels (tests/emu_build.py): image sizes that are no multiple of the store's 16 x 8 tiles,
of a workgroup's footprint or of anything else, levels down to a few pixels, grid cells larger than the image, frames with
9 ... 520 patches (every workgroup size of K1, at both of its widths) -- each against the oracle, bit for bit where the GPU tests ask for that.  The
border arithmetic is where an out-of-bounds access would hide: scripts/emu_sanitize.sh runs this file under
AddressSanitizer, too."""
import numpy as np
import pytest

import k1_cases as k1
import k1_emulated
from oracle import pytrack
from rpg_svo_amd import capi, synth
from test_fast_emulated import detect
from test_pyramid_emulated import HostStore, _check


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.mark.parametrize("w,h", [(17, 16), (16, 16), (31, 33), (64, 8), (100, 37), (129, 65), (255, 254), (333, 17), (48, 480), (640, 2),
                                 (18, 130), (97, 97)])
def test_pyramid_of_any_shape(emu, oracle, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    for levels in (1, 2, 3, 4, 5):
        if (w >> (levels - 1)) < 1 or (h >> (levels - 1)) < 1:
            continue
        imgs = rng.integers(0, 256, size=(3, h, w), dtype=np.uint8)
        for path in ("fused", "from_store", "per_level", "upload"):
            st = HostStore(emu, w, h, levels, 4)
            st.buf[:] = 0xEE
            if path == "fused":
                st.load_images(imgs, first_slot=1)
            elif path == "from_store":
                st.load_images(imgs, first_slot=1, fused=False)
            elif path == "per_level":
                st.load_images(imgs, first_slot=1, build=False)
                st.build_per_level(1, 3)
            else:
                for i in range(3):
                    st.upload(1 + i, imgs[i])
            _check(st, oracle, imgs, levels, capi.HALFSAMPLE_AUTO, 1)


@pytest.mark.parametrize("w,h,levels,cell", [(64, 48, 1, 30), (97, 61, 2, 25), (130, 18, 2, 10), (33, 200, 3, 32), (255, 254, 4, 30),
                                             (48, 40, 3, 7), (160, 120, 3, 200), (31, 33, 1, 5)])
def test_fast_on_any_shape(emu, oracle, w, h, levels, cell):
    rng = np.random.default_rng(w + h)
    imgs = rng.integers(0, 256, size=(2, h, w), dtype=np.uint8)
    imgs[1] = (np.add.outer(np.arange(h) // 5, np.arange(w) // 7) % 2 * 200 + 20).astype(np.uint8)   # corners everywhere
    cols, rows = -(-w // cell), -(-h // cell)
    occ = (rng.uniform(size=(2, cols * rows)) < 0.2).astype(np.uint8)
    xy, lvl, sc, cols, rows = detect(emu, imgs, levels, levels, cell, occ)
    for i in range(2):
        pyr = oracle.create_img_pyramid(imgs[i], levels)
        exy, elvl, esc, n = pytrack.fast_detect_grid(pyr, levels, cell, cols, rows, occ[i], 20, 20.0)
        assert np.array_equal(sc[i].view(np.uint32), esc.view(np.uint32))
        assert np.array_equal(xy[i], exy) and np.array_equal(lvl[i], elvl)


@pytest.fixture(scope="module")
def k1_default():
    return k1_emulated.Emulated(0)


@pytest.fixture(scope="module")
def k1_reference_width():
    """the reference-width build of K1 (emu_build.BUILDS[2]: -DSIA_F64_PARTIALS)"""
    return k1_emulated.Emulated(2)


def _sparse_align_on_a_shape(backend, oracle, w, h, n):
    c = k1.case(f"shape_{w}x{h}_n{n}")
    k1.verify_pair(oracle, backend.name, c.name, c.schedules[0], backend.run(c, c.schedules[0]))


@pytest.mark.parametrize("w,h,n,levels,lo,hi", k1.SHAPES)
def test_sparse_align_on_any_shape(k1_default, oracle, w, h, n, levels, lo, hi):
    """(64-, 128-, 256-, 512- and 1024-lane workgroups; a frame with a third of the patches in the middle of the batch -- 513 of
    520 for the 1024-lane one, so that it stays above 512)"""
    _sparse_align_on_a_shape(k1_default, oracle, w, h, n)


@pytest.mark.parametrize("w,h,n,levels,lo,hi", k1.SHAPES)
def test_sparse_align_on_any_shape_at_reference_width(k1_reference_width, oracle, w, h, n, levels, lo, hi):
    """the same shapes and asserts on the -DSIA_F64_PARTIALS build: f64 products and SE3::exp, the scalar pixel loop, in every
    workgroup size"""
    _sparse_align_on_a_shape(k1_reference_width, oracle, w, h, n)


@pytest.mark.parametrize("kind", ["pinhole", "atan"])
def test_matcher_and_depth_filter_on_an_odd_image_size(emu, oracle, kind):
    """find_match_direct and update_seeds (tests/test_track_emulated.py) on 438 x 410 images: 27.4 x 51.25 tiles of the store"""
    import tracking_cases as tc
    import tracking_emulated as te
    cam = synth.Camera(438, 410, 260.0, 260.0, 219.0, 205.0) if kind == "pinhole" else \
        synth.Camera.atan(438, 410, 0.509326, 0.796651, 0.45905, 0.510056, 0.9320)
    scene = synth.make_track_scene(n_kf=4, n_feat=100, cam=cam)
    c = tc.of_scene(scene, "odd size")
    tc.verify_matcher(c, *te.find_match_direct(emu, c))
    n_ok, n_edge = tc.matcher_coverage(c)
    assert n_ok > 200 and n_edge > 20
    first = te.update_seeds(emu, c, 0, 1, 1000)
    order = tc.seed_order(c)
    tc.verify_seed_order(order, first, te.update_seeds(emu, c, 0, 1, 1000, order))
    tc.verify_seeds(c, 0, 1, 1000, *first)
    tc.seed_coverage(c)
