"""Keyed noise on the host (no GPU needed): the numpy mirror of the integer part of include/mbexwn_noise.h's definition
(mbexwn_vocoder_amd/noise.py) against the published known answers of Philox4x32-10, its float64 evaluation of the normals,
and the header, export and refusals of mbxn_fill_normal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mbexwn_vocoder_amd import noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFF


def hexes(words):
    return " ".join(f"{int(ww):08x}" for ww in words)


def test_philox_known_answers():
    """The vectors of the Random123 distribution (kat_vectors, philox4x32 10): zero, all ones, and the digits of pi."""
    assert hexes(noise.philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(noise.philox4x32_10([ONES] * 4, [ONES] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(noise.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over quads: the rows of a batch are the single calls
    both = noise.philox4x32_10([[0, 0, 0, 0], [ONES] * 4], [[0, 0], [ONES] * 2])
    assert both.dtype == np.uint32 and both.shape == (2, 4)
    assert hexes(both[0]).startswith("6627e8d5") and hexes(both[1]).startswith("408f276d")


def test_counter_high_word_and_window_indexing():
    """Quad q = 2^32 + 5 has a non-zero high counter word and differs from q = 5; a window is a slice of the whole."""
    lo, hi = noise.words(3, 9, 4 * 5, 4), noise.words(3, 9, 4 * ((1 << 32) + 5), 4)
    k0, k1 = noise.philox_key(3, 9)
    assert np.array_equal(lo, noise.philox4x32_10([5, 0, 0, 0], [k0, k1]))
    assert np.array_equal(hi, noise.philox4x32_10([5, 1, 0, 0], [k0, k1]))
    assert not np.array_equal(lo, hi)
    whole = noise.words(3, 9, 0, 64)
    for first, count in ((1, 2), (3, 9), (4, 4), (7, 50), (63, 1), (10, 0)):
        assert np.array_equal(noise.words(3, 9, first, count), whole[first:first + count])
    base = (1 << 34) + 3
    assert np.array_equal(noise.words(3, 9, base, 7), noise.words(3, 9, base - 3, 10)[3:])
    with pytest.raises(ValueError):
        noise.words(3, 9, -1, 4)


def test_keys_and_seeds_give_different_streams_and_item_key_is_stable():
    aa = noise.words(0, 1, 0, 256)
    assert not np.array_equal(aa, noise.words(0, 2, 0, 256))
    assert not np.array_equal(aa, noise.words(1, 1, 0, 256))
    assert np.array_equal(aa, noise.words(0, 1, 0, 256))
    # k = seed ^ (item_key * 0x9E3779B97F4A7C15 mod 2^64): low and high words
    assert noise.philox_key(0, 1) == (0x7F4A7C15, 0x9E3779B9)
    assert noise.philox_key(0xFFFFFFFF00000000, 1) == (0x7F4A7C15, 0x9E3779B9 ^ ONES)
    assert noise.philox_key(5, 0) == (5, 0)
    assert noise.philox_key(-1, 0) == (ONES, ONES)                      # seeds are taken mod 2^64
    # zlib.crc32 of the basename's UTF-8 bytes: the directory does not count, the extension does
    assert noise.item_key("utt0.mell") == 479674467
    assert noise.item_key("a.wav") == noise.item_key("/x/y/a.wav") == noise.item_key(os.path.join("rel", "a.wav")) == 3064168919
    assert noise.item_key("a.wav") != noise.item_key("a.flac")
    assert noise.item_key("é.wav") == __import__("zlib").crc32("é.wav".encode("utf-8"))
    assert noise.item_key(17) == 17 and noise.item_key(np.int64(17)) == 17


def test_uniforms_lie_strictly_inside_the_unit_interval_and_are_exact_in_float32():
    edge = noise.unit_open(np.array([0, ONES, 0x1FF, 0x200], dtype=np.uint32))
    assert edge[0] == 2.0 ** -24 and edge[1] == 1 - 2.0 ** -24 and edge[2] == edge[0] and edge[3] == 3 * 2.0 ** -24
    assert np.all(edge > 0) and np.all(edge < 1)
    uu = noise.uniforms(11, noise.item_key("a.wav"), 5, 1 << 16)
    assert uu.dtype == np.float64 and uu.shape == (1 << 16,)
    assert np.all(uu > 0) and np.all(uu < 1)
    assert np.array_equal(uu.astype(np.float32).astype(np.float64), uu)          # no rounding on the way to float32
    assert np.all(edge.astype(np.float32) < np.float32(1)) and np.all(edge.astype(np.float32) > 0)


def test_normals_reference_has_the_moments_of_a_standard_normal():
    """2^20 values: |mean| < 0.005, |var - 1| < 0.01, |excess kurtosis| < 0.05 -- about five standard errors each
    (1 / sqrt(n) = 0.00098, sqrt(2 / n) = 0.0014, sqrt(24 / n) = 0.0048)."""
    nn = 1 << 20
    zz = noise.normals_reference(7, noise.item_key("a.wav"), 0, nn)
    assert zz.dtype == np.float64 and zz.shape == (nn,) and np.all(np.isfinite(zz))
    mean, var = zz.mean(), zz.var()
    kurt = np.mean((zz - mean) ** 4) / var ** 2 - 3.0
    print(f"mean {mean:.5f} var {var:.5f} excess kurtosis {kurt:.5f}")
    assert abs(mean) < 0.005 and abs(var - 1) < 0.01 and abs(kurt) < 0.05
    assert np.max(np.abs(zz)) <= np.sqrt(-2 * np.log(2.0 ** -24))               # the radius of the smallest uniform
    # a window is a slice of the whole, also one that starts or ends inside a pair or a quad
    for first, count in ((1, 1), (2, 5), (3, 130), (4095, 6), (0, 0)):
        assert np.array_equal(noise.normals_reference(7, noise.item_key("a.wav"), first, count), zz[first:first + count])
    # the float32 port of the same formulas stays within float32 rounding of it
    port = noise.normals_float32_port(7, noise.item_key("a.wav"), 0, nn)
    assert port.dtype == np.float32 and np.max(np.abs(port - zz)) < 4e-6


def test_header_declares_the_fill_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    path = os.path.join(ROOT, "include", "mbexwn_noise.h")
    text = open(path).read()
    assert "Philox4x32-10" in text and "Refused" in text and "first_step" in text      # the definition, the refusals, the buffers
    assert abi.symbols("mbexwn_noise.h") == ["mbxn_fill_normal"]
    assert any(hh.endswith("mbexwn_noise.h") for hh in HEADERS) and "noise_keyed.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_noise.h"\nint main(void){ (void)mbxn_fill_normal; return MBXN_FILL_TILE == 4096 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_fill_refuses_bad_arguments_before_touching_the_device():
    """mbxn_fill_normal checks every argument on the host and returns MBX_ERR_INVALID_ARGUMENT without a launch."""
    from mbexwn_vocoder_amd import engine
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = engine.load_library()
    fake = ctypes.c_void_p(256)                              # never dereferenced: the checks fail first

    def call(stride=4096, batch=2, max_count=100, out=fake, keys=fake, counts=fake, first=None):
        return lib.mbxn_fill_normal(out, stride, batch, keys, first, counts, max_count, None)

    def why():
        return lib.mbx_last_error().decode()

    for name in ("out", "keys", "counts"):
        assert call(**{name: None}) == 1 and why().startswith("fill normal:") and "null" in why(), name
    for name in ("batch", "stride", "max_count"):
        assert call(**{name: -1}) == 1 and why().startswith("fill normal:") and "negative" in why(), name
    assert call(stride=99, max_count=100) == 1 and why().startswith("fill normal:") and "stride" in why()
    assert call(stride=1 << 40, batch=(1 << 31) - 1, max_count=1 << 30) == 1 and "tiles" in why()
    assert call(batch=0) == 0                                # an empty batch is nothing to do
    assert call(max_count=0) == 0 and call(stride=0, max_count=0) == 0      # no values: nothing is launched
