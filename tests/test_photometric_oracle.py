"""The numpy restatement of the photometric augmentations (tests/photometric_oracle.py) against the installed
Pillow, which runs the same C arithmetic the reference's PIL calls ran: blend (brightness / contrast /
saturation), the contrast mean, the HSV round trip on every RGB value, and the extended box blur."""
import numpy as np
import pytest

from tests import photometric_oracle as PH

Image = pytest.importorskip('PIL.Image')
from PIL import ImageEnhance, ImageFilter  # noqa: E402


def _pil(x):
    return Image.fromarray(np.ascontiguousarray(x), 'RGB')


def _all_values():
    v = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(-1, 3)


@pytest.mark.parametrize('lo,hi', [(0.6, 1.4)])
def test_blend_matches_pillow(lo, hi):
    g = np.random.default_rng(0)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, -1)
    ramp[..., 1] = ramp[..., 1][:, ::-1]
    ramp[..., 2] = np.roll(ramp[..., 2], 77, axis=1)
    x = np.ascontiguousarray(ramp)
    factors = np.concatenate([g.uniform(lo, hi, 1000), [0.0, 1.0, lo, hi]])
    for f in factors:
        assert np.array_equal(PH.adjust_brightness(x, f), np.asarray(ImageEnhance.Brightness(_pil(x)).enhance(f))), f
        assert np.array_equal(PH.adjust_saturation(x, f), np.asarray(ImageEnhance.Color(_pil(x)).enhance(f))), f
        d = int(g.integers(0, 256))
        want = Image.blend(Image.new('RGB', (256, 1), (d, d, d)), _pil(x), float(f))
        assert np.array_equal(PH.blend(x, d, f), np.asarray(want)), (f, d)


def test_contrast_mean_matches_pillow():
    g = np.random.default_rng(1)
    for k in range(200):
        h, w = int(g.integers(1, 40)), int(g.integers(1, 40))
        x = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 3 == 0:
            x = np.clip(x.astype(np.int32) // 4 + int(g.integers(0, 192)), 0, 255).astype(np.uint8)
        f = float(g.uniform(0.6, 1.4))
        assert np.array_equal(PH.adjust_contrast(x, f), np.asarray(ImageEnhance.Contrast(_pil(x)).enhance(f))), (k, f)


def test_hsv_round_trip_matches_pillow_on_every_value():
    rgb = _all_values().reshape(4096, 4096, 3)
    hsv = np.asarray(_pil(rgb).convert('HSV'))
    assert np.array_equal(PH.rgb2hsv(rgb), hsv)
    back = np.asarray(Image.frombytes('HSV', (4096, 4096), rgb.tobytes()).convert('RGB'))
    assert np.array_equal(PH.hsv2rgb(rgb), back)


def test_hue_matches_torchvision_07_recipe():
    """adjust_hue of torchvision 0.7: HSV split, H += np.uint8(factor*255) wrapping, merge, back to RGB"""
    g = np.random.default_rng(2)
    x = g.integers(0, 256, (32, 48, 3), dtype=np.uint8)
    for f in list(g.uniform(-0.1, 0.1, 40)) + [-0.5, -0.1, 0.0, 0.1, 0.5]:
        h, s, v = _pil(x).convert('HSV').split()
        nh = ((np.asarray(h).astype(np.int32) + PH.hue_shift(float(f))) & 255).astype(np.uint8)
        want = Image.merge('HSV', (Image.fromarray(nh, 'L'), s, v)).convert('RGB')
        assert np.array_equal(PH.adjust_hue(x, float(f)), np.asarray(want)), f
    assert PH.hue_shift(-0.1) == 231 and PH.hue_shift(0.1) == 25 and PH.hue_shift(0.0) == 0


def test_blur_matches_pillow():
    g = np.random.default_rng(3)
    shapes = [(23, 31), (1, 9), (9, 1), (1, 1), (2, 2), (16, 17)]
    sigmas = list(g.uniform(0.1, 0.2, 300)) + [0.1, 0.2]
    for k, s in enumerate(sigmas):
        h, w = shapes[k % len(shapes)]
        x = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(_pil(x).filter(ImageFilter.GaussianBlur(radius=float(s))))
        assert np.array_equal(PH.gaussian_blur(x, float(s)), want), (k, s)
    with pytest.raises(NotImplementedError):
        PH.blur_weights(2.0)


def test_jitter_check_input():
    assert PH.jitter_ranges(0.4, 0.4, 0.4, 0.1) == [[0.6, 1.4], [0.6, 1.4], [0.6, 1.4], [-0.1, 0.1]]
    assert PH.jitter_ranges() == [None, None, None, None]
    assert PH.jitter_ranges(brightness=1.5)[0] == [0.0, 2.5]
    assert PH.jitter_ranges(contrast=(1, 1))[1] is None and PH.jitter_ranges(hue=(0.0, 0.0))[3] is None
    with pytest.raises(ValueError):
        PH.jitter_ranges(hue=0.7)
    with pytest.raises(ValueError):
        PH.jitter_ranges(saturation=-1)
