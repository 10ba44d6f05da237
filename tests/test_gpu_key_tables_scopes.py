"""The launches of the clip batches with a key per clip (K16 and K16g, hip/keytab.hip), pinned.

The bit comparisons of test_gpu_parity.py see what a call writes; they cannot see HOW: which scopes it opened, how many launches each scope
counted and which byte count it was given.  This file holds that table, for one call per form, to tests/golden/key_tables_scopes.json, for
equality.  The forms:

  add_watermark_batch_keys   3 clips and 257 clips (one more than a launch of K16 and a group of keys) of 1024 + 37 i frames, with
                             awm_debug_set_add_batched 0, 1 and 2 and the tables from the device, and 2 with the tables from the host
                             (257 crosses that path's 128 tables per upload twice)
  get_watermark_batch_keys   65 clips of one second (one more than a clip group) on one host thread, with
                             awm_debug_set_key_tables_on_device 0, 1 and 2

Stereo noise; one call per form to warm up (what a context makes once is made there), then the measured one.

The golden file is a recording: AWM_RECORD_KEY_TABLES_SCOPES=<path> makes the module write what it observed to <path>.  It is recorded on
the commit BEFORE a change to the host side of these paths and must not change with it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_tables_scopes.json")
RECORD = "AWM_RECORD_KEY_TABLES_SCOPES"
PAYLOAD = "0123456789abcdef0011223344556677"

# (entry point, clips, awm_debug_set_add_batched, awm_debug_set_key_tables_on_device)
FORMS = [("add", n, batched, 1) for n in (3, 257) for batched in (0, 1, 2)] + [("add", n, 2, 0) for n in (3, 257)] \
      + [("get", 65, 2, on_device) for on_device in (0, 1, 2)]


def form_name(form):
    return "%s-%d_clips-batched_%d-on_device_%d" % form


@pytest.fixture(scope="module")
def observed():
    """{form: {scope: [launches, algorithmic bytes]}} of one call per form, the scopes that counted anything"""
    import torch
    import audiowmark_amd as awm
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    ctx = awm.Context(0)
    lib = awm.lib
    lib.awm_prof_name.restype = C.c_char_p
    rng = np.random.default_rng(1616)
    add_clips = [torch.from_numpy(rng.uniform(-1, 1, (1024 + 37 * i, 2)).astype(np.float32)).cuda() for i in range(257)]
    get_clips = [torch.from_numpy(rng.uniform(-1, 1, (44100, 2)).astype(np.float32)).cuda() for i in range(65)]
    keys = [awm.test_key(1 + i) for i in range(257)]

    def call(form):
        entry, n, batched, on_device = form
        lib.awm_debug_set_add_batched(batched)
        lib.awm_debug_set_key_tables_on_device(on_device)
        if entry == "add":
            return ctx.add_watermark_batch_keys(keys[:n], PAYLOAD, add_clips[:n])
        return ctx.get_watermark_batch_keys(keys[:n], get_clips[:n], n_threads=1)

    table = {}
    try:
        for form in FORMS:
            call(form)
            ctx.synchronize()
            lib.awm_prof_enable(ctx._h, 1)
            try:
                lib.awm_prof_reset(ctx._h)
                call(form)
                ctx.synchronize()
                scopes = {}
                for i in range(lib.awm_prof_count()):
                    launches, nbytes = C.c_long(), C.c_double()
                    assert lib.awm_prof_read(ctx._h, i, None, C.byref(launches), C.byref(nbytes)) == 0
                    if launches.value or nbytes.value:
                        scopes[lib.awm_prof_name(i).decode()] = [launches.value, nbytes.value]
            finally:
                lib.awm_prof_enable(ctx._h, 0)
            table[form_name(form)] = scopes
    finally:
        lib.awm_debug_set_add_batched(2)
        lib.awm_debug_set_key_tables_on_device(1)
        ctx.close()
    if os.environ.get(RECORD):
        with open(os.environ[RECORD], "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    return table


@pytest.mark.parametrize("form", FORMS, ids=form_name)
def test_scopes_as_recorded(observed, form):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(form_name(f) for f in FORMS)
    assert observed[form_name(form)] == golden[form_name(form)]


def test_the_tables_come_from_where_the_form_says(observed):
    """(what is pinned is K16's and K16g's launch structure: the forms with the tables from the device count key-table launches, the
    others none)"""
    for form in FORMS:
        assert ("frame_mod_table_kernel" in observed[form_name(form)]) == (form[3] != 0), form_name(form)
