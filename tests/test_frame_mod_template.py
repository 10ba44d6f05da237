"""The key template of the frame_mod tables (awm_tab_frame_mod_template; host/wmcommon.cc build_frame_mod_template).

For one key the tables of two payloads differ only in UP <-> DOWN of the data bands (reference wmadd.cc:86-162), so a payload's table is
a pure function of a key-only template and the 2 x 858 coded bits of the payload.  K16p (hip/keytab.hip) does that expansion on the
device; here numpy does it, with awm_conv_encode's A and B code, and the result must be awm_tab_frame_mod byte for byte.  No GPU."""
import numpy as np
import pytest

import audiowmark_amd as awm

N_CODE = 858
KEYS = [None, awm.test_key(1), awm.test_key(42)]
PAYLOADS = ["0123456789abcdef0011223344556677", "ffffffffffffffffffffffffffffffff", "a5"]
GEOMETRIES = [dict(), dict(mix=False), dict(frames_per_bit=1), dict(frames_per_bit=3)]
GEOMETRY_IDS = ["default", "linear", "frames_per_bit1", "frames_per_bit3"]


def payload_bits(payload_hex):
    """parse_payload: the bits of the hex string, most significant first, repeated up to 128"""
    bits = [(int(c, 16) >> (3 - i)) & 1 for c in payload_hex for i in range(4)]
    return np.array([bits[i % len(bits)] for i in range(128)], np.int32)


def expand(template, payload_hex):
    """what K16p computes: 0 / 1 / 2 as they are, 4 + 2 k + s -> UP (1) if bit k of the block type's code xor s, else DOWN (2)"""
    out = np.empty(template.shape, np.int8)
    for ab in range(2):
        code = awm.conv_encode(ab, payload_bits(payload_hex))
        assert code.shape == (N_CODE,)
        t = template[ab].astype(np.int32)
        data = t >= 4
        k, s = (t - 4) >> 1, (t - 4) & 1
        bit = code[np.where(data, k, 0)]
        out[ab] = np.where(data, 2 - (bit ^ s), t)
    return out


@pytest.fixture(params=GEOMETRIES, ids=GEOMETRY_IDS)
def geometry(request):
    awm.set_params(**request.param)
    try:
        yield 510 + N_CODE * request.param.get("frames_per_bit", 2)
    finally:
        awm.set_params()


def tab_frame_mod(key, payload_hex, block_frames):
    out = np.zeros((2, block_frames, awm.N_BANDS), np.int8)
    n = awm.lib.awm_tab_frame_mod(awm.key_bytes(key), payload_hex.encode(), out.ctypes.data)
    assert n == out.size
    return out


@pytest.mark.parametrize("key", KEYS, ids=["key0", "key1", "key42"])
def test_expanded_template_is_the_table(geometry, key):
    template = awm.frame_mod_template(key, geometry)
    assert template.shape == (2, geometry, awm.N_BANDS) and template.dtype == np.int16
    for payload in PAYLOADS:
        assert np.array_equal(expand(template, payload), tab_frame_mod(key, payload, geometry)), payload


@pytest.mark.parametrize("key", KEYS, ids=["key0", "key1", "key42"])
def test_template_entries(geometry, key):
    """every entry is 0, 1, 2 or 4 + 2 k + s with k < 858; per block type every k occurs, as often with s = 0 as with s = 1"""
    template = awm.frame_mod_template(key, geometry).astype(np.int64)
    assert template.min() >= 0 and not (template == 3).any()
    assert template.max() < 4 + 2 * N_CODE
    for ab in range(2):
        data = template[ab][template[ab] >= 4] - 4
        k, s = data >> 1, data & 1
        up = np.bincount(k[s == 0], minlength=N_CODE)
        down = np.bincount(k[s == 1], minlength=N_CODE)
        assert (up > 0).all() and np.array_equal(up, down)
        # the sync frames: 510 frames x 30 bands up and as many down, whatever the geometry
        assert (template[ab] == 1).sum() == (template[ab] == 2).sum() == 510 * 30


def test_template_differs_by_key_and_block_type():
    a, b = awm.frame_mod_template(KEYS[1]), awm.frame_mod_template(KEYS[2])
    assert not np.array_equal(a, b)
    # A and B carry inverse sync sequences and the same data bands
    assert np.array_equal(a[0] >= 4, a[1] >= 4) and np.array_equal(a[0][a[0] >= 4], a[1][a[1] >= 4])
    sync = (a[0] == 1) | (a[0] == 2)
    assert np.array_equal(a[0][sync], 3 - a[1][sync])


def test_template_is_sized_by_the_parameters_in_force(geometry):
    """the buffer follows the geometry in force, not the caller: no block_frames gives the right shape, another one is refused"""
    assert awm.frame_mod_template(KEYS[1]).shape == (2, geometry, awm.N_BANDS)
    assert awm.lib.awm_tab_frame_mod_template(awm.key_bytes(KEYS[1]), None) == 2 * geometry * awm.N_BANDS
    with pytest.raises(ValueError, match="block_frames"):
        awm.frame_mod_template(KEYS[1], geometry + 858)
