"""The launches of the segment batches of `add` (DESIGN.md sections 9.2, 9.3, 9.6, 9.7, 9.8), pinned.

The bit comparisons of test_gpu_add_segments*.py see what a call writes; they cannot see HOW: which scopes it opened, how many launches
each scope counted and which byte count it was given.  This file holds that table for one small fixed stereo batch through all twelve
forms -- {float, 16-bit} x {one key, a key each} x {all 44100, all 48000, a rate each} -- to tests/golden/add_segments_scopes.json, for
equality, together with awm_debug_add_segments_fused_in_use().

The batch: eight segments of 0, 1, 1023, 1025, 2048, 5000, 5000, 5000 samples at 0, 1, 1024, 513, 44100 * 600 and three times
44100 * 600 + 513 samples into their streams (1, 513 and 26460513 are no multiples of 1024: staged at 44.1 kHz); the last three are one
input with one length and offset (a shared down slice where their rates agree); three payloads, two keys.

The golden file is a recording: AWM_RECORD_ADD_SEGMENTS_SCOPES=<path> makes the module write what it observed to <path>.  It is recorded on
the commit BEFORE a change to the host side of these entry points and must not change with it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "add_segments_scopes.json")
RECORD = "AWM_RECORD_ADD_SEGMENTS_SCOPES"

LENGTHS = [0, 1, 1023, 1025, 2048, 5000, 5000, 5000]
ZERO_FRAMES = [0, 1, 1024, 513, 44100 * 600, 26460513, 26460513, 26460513]
MIXED = [48000, 44100, 32000, 48000, 44100, 22050, 48000, 48000]
RATES = {"44100": 44100, "48000": 48000, "mixed": MIXED}
PAYLOAD_OF = [0, 1, 2, 2, 1, 0, 1, 1]
KEY_OF = [0, 1, 1, 0, 0, 1, 0, 1]
FORMS = [(sample, keys, rates) for sample in ("float", "s16") for keys in ("one_key", "key_each") for rates in ("44100", "48000", "mixed")]


def form_name(form):
    return "-".join(form)


def payloads():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, 16, dtype=np.uint8).tobytes().hex() for _ in range(3)]


@pytest.fixture(scope="module")
def observed():
    """{form: {"fused": 0 | 1, "scopes": {scope: [launches, algorithmic bytes]}}} of one call per form, the scopes that counted anything"""
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    assert 26460513 == 44100 * 600 + 513
    ctx = awm.Context(0)
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2024)
    inputs = [((torch.rand((n, 2), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1) * 0.98).contiguous() for n in LENGTHS[:6]]
    inputs += [inputs[5], inputs[5]]
    inputs16 = {id(x): torch.round(x * 32767).to(torch.int16).contiguous() for x in inputs}
    pays = [payloads()[p] for p in PAYLOAD_OF]
    two_keys = [None, bytes(range(16))]

    def call(form):
        sample, keys, rates = form
        segs = inputs if sample == "float" else [inputs16[id(x)] for x in inputs]
        suffix = "" if sample == "float" else "_s16"
        if keys == "one_key":
            return getattr(ctx, "add_watermark_segments" + suffix)(None, pays, segs, ZERO_FRAMES, sample_rate=RATES[rates])
        return getattr(ctx, "add_watermark_segments_keys" + suffix)([two_keys[k] for k in KEY_OF], pays, segs, ZERO_FRAMES, sample_rate=RATES[rates])

    table = {}
    try:
        for form in FORMS:
            call(form)                                     # (tables and templates that a context makes once are made here)
            ctx.synchronize()
            lib.awm_prof_enable(ctx._h, 1)
            try:
                lib.awm_prof_reset(ctx._h)
                call(form)
                fused = awm.add_segments_fused_in_use()
                ctx.synchronize()
                scopes = {}
                for i in range(lib.awm_prof_count()):
                    launches, nbytes = C.c_long(), C.c_double()
                    assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), C.byref(nbytes)) == 0
                    if launches.value or nbytes.value:
                        scopes[lib.awm_prof_name(i).decode()] = [launches.value, nbytes.value]
            finally:
                lib.awm_prof_enable(ctx._h, 0)
            table[form_name(form)] = {"fused": fused, "scopes": scopes}
    finally:
        ctx.close()
    if os.environ.get(RECORD):
        with open(os.environ[RECORD], "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    return table


@pytest.mark.parametrize("form", FORMS, ids=form_name)
def test_scopes_and_path_as_recorded(observed, form):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(form_name(f) for f in FORMS)
    assert observed[form_name(form)] == golden[form_name(form)]


def test_the_batch_takes_the_fused_path_in_every_form(observed):
    """(what is pinned is the fused paths' launch structure, not the fallback's)"""
    assert all(entry["fused"] == 1 and entry["scopes"] for entry in observed.values())
