"""ctypes binding of include/awm_hip.h.  Names follow the reference's operators:
add_watermark / get_watermark (wmcommon.hh:226-228), SyncFinder.search, fft_range, ..."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
N_BANDS = 81
BLOCK_FRAMES = 2226
SOFT_BITS = 858


class AwmError(RuntimeError):
    pass


def library_path():
    return os.path.join(_HERE, "libawm_hip.so")


# (Runtime settings are the application's business, not this module's: a process that wants every lane of `get` on a hardware
# queue of its own exports GPU_MAX_HW_QUEUES=16 before its first HIP call -- bench.py and tests/conftest.py do.)


def _load_hip_runtime():
    """libawm_hip.so has no DT_NEEDED on a HIP runtime: bind it to the runtime of this process.  PyTorch
    ships its own libamdhip64.so (no SONAME) next to libtorch_hip.so; a second runtime in the same process
    cannot open the KFD device, so torch's copy is preferred and made global before our library is loaded."""
    candidates = []
    try:
        import torch
        candidates.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:
        pass
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    candidates += [os.path.join(rocm, "lib", "libamdhip64.so.7"), os.path.join(rocm, "lib", "libamdhip64.so")]
    for c in candidates:
        if os.path.exists(c):
            return C.CDLL(c, mode=C.RTLD_GLOBAL)
    raise AwmError("no HIP runtime (libamdhip64) found for libawm_hip.so")


def _load():
    path = library_path()
    if not os.path.exists(path):
        raise AwmError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C audiowmark_amd/csrc` (there is no CPU fallback)")
    _load_hip_runtime()
    return C.CDLL(path)


class Pattern(C.Structure):
    _fields_ = [("time", C.c_double), ("sync_index", C.c_uint64), ("sync_quality", C.c_double),
                ("block_type", C.c_int), ("type", C.c_int), ("decode_error", C.c_float), ("speed", C.c_double),
                ("bits", C.c_int * 128), ("n_bits", C.c_int)]

    def hex(self):
        b = list(self.bits[:self.n_bits])
        return "".join("%x" % (b[i] * 8 + b[i + 1] * 4 + b[i + 2] * 2 + b[i + 3]) for i in range(0, len(b) - 3, 4))

    def as_dict(self):
        return dict(time=self.time, sync_index=int(self.sync_index), sync_quality=self.sync_quality,
                    block_type=self.block_type, type=self.type, decode_error=self.decode_error, speed=self.speed,
                    bits=self.hex())


_HEX = np.frombuffer(b"0123456789abcdef", np.uint8)


def patterns_to_dicts(buf, count, first=0):
    """The first `count` entries of a ctypes Pattern array as dicts (Pattern.as_dict for each, vectorised: the payload
    hex strings are built with numpy instead of 128 Python operations per pattern)."""
    if count <= 0:
        return []
    if isinstance(buf, np.ndarray):
        a = buf[first:first + count]
    else:
        a = np.frombuffer(buf, dtype=np.dtype(Pattern), count=count, offset=first * C.sizeof(Pattern))
    bits = a["bits"].astype(np.uint8)
    nib = (bits[:, 0::4] << 3) | (bits[:, 1::4] << 2) | (bits[:, 2::4] << 1) | bits[:, 3::4]
    text = _HEX[nib]                                   # [count, 32] ASCII
    n_hex = (a["n_bits"] // 4).tolist()
    rows = text.tobytes().decode()
    w = text.shape[1]
    cols = [a[f].tolist() for f in ("time", "sync_index", "sync_quality", "block_type", "type", "decode_error", "speed")]
    return [dict(time=t, sync_index=si, sync_quality=sq, block_type=bt, type=ty, decode_error=de, speed=sp,
                 bits=rows[i * w:i * w + n_hex[i]])
            for i, (t, si, sq, bt, ty, de, sp) in enumerate(zip(*cols))]


lib = _load()
_u8p = C.POINTER(C.c_uint8)
_vp = C.c_void_p
lib.awm_last_error.restype = C.c_char_p
lib.awm_version.restype = C.c_char_p
lib.awm_ctx_stream.restype = C.c_void_p
lib.awm_search_approx_d.restype = C.c_long
lib.awm_set_params.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double]
lib.awm_set_params.restype = None
lib.awm_ctx_create.argtypes = [C.c_int, C.POINTER(_vp)]
lib.awm_ctx_destroy.argtypes = [_vp]
lib.awm_ctx_destroy.restype = None
lib.awm_ctx_synchronize.argtypes = [_vp]
lib.awm_ctx_stream.argtypes = [_vp]
lib.awm_ctx_set_stream.argtypes = [_vp, _vp]
lib.awm_stft_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, _vp]
lib.awm_add_init_block_max_d.argtypes = [_vp, _vp, C.c_size_t]
lib.awm_add_mix_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_double, C.c_size_t, _vp, _vp, _vp,
                              C.c_size_t, C.c_size_t]
lib.awm_add_limit_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t, _vp, C.c_size_t, C.c_size_t]
lib.awm_add_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_double, C.c_int]
lib.awm_sync_fft_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp]
lib.awm_sync_search_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, _vp, _vp, _vp]
lib.awm_search_approx_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, _vp, _vp, _vp]
lib.awm_block_soft_bits_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, _vp, _vp]
lib.awm_viterbi_decode.argtypes = [_vp, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, _vp]
lib.awm_add_watermark_d.argtypes = [_vp, _vp, C.c_char_p, _vp, _vp, C.c_size_t, C.c_int, C.c_int]
lib.awm_get_watermark_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, _vp]
lib.awm_add_get_watermark_d.argtypes = [_vp, _vp, C.c_char_p, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, _vp]
lib.awm_resample_frames.argtypes = [_vp, C.c_size_t, C.c_int, C.c_int]
lib.awm_resample_frames.restype = C.c_size_t
lib.awm_resample_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t]
lib.awm_add_watermark_payloads_d.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_int]
lib.awm_debug_set_add_payloads_fused.argtypes = [C.c_int]
lib.awm_debug_set_add_payloads_fused.restype = None
lib.awm_debug_add_payloads_fused_in_use.argtypes = []
lib.awm_debug_add_payloads_fused_in_use.restype = C.c_int
lib.awm_debug_set_add_payloads_rate_fused.argtypes = [C.c_int]
lib.awm_debug_set_add_payloads_rate_fused.restype = None
lib.awm_debug_add_payloads_rate_fused_in_use.argtypes = []
lib.awm_debug_add_payloads_rate_fused_in_use.restype = C.c_int
lib.awm_debug_add_payloads_tile.argtypes = []
lib.awm_debug_add_payloads_tile.restype = C.c_int
lib.awm_add_watermark_batch_d.argtypes = [_vp, _vp, C.c_char_p, C.c_size_t, _vp, _vp, _vp, C.c_int]
lib.awm_add_watermark_segments_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int]
lib.awm_add_watermark_segments_rate_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]
lib.awm_add_watermark_segments_keys_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int]
lib.awm_add_watermark_segments_keys_rate_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]
lib.awm_add_watermark_segments_rate_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]
lib.awm_add_watermark_segments_keys_rate_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]
lib.awm_add_watermark_segments_rates_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
lib.awm_add_watermark_segments_keys_rates_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
lib.awm_add_watermark_segments_rates_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
lib.awm_add_watermark_segments_keys_rates_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]


class SegmentPlan(C.Structure):
    """awm_segment_plan (include/awm_hip.h): the window of one stream segment at another sample rate"""
    _fields_ = [(n, C.c_uint64) for n in ("mix_first", "frame_first", "frame_last", "slice_first", "slice_last", "down_first", "down_last",
                                          "in_first", "in_last", "limiter_block", "first_block", "n_blocks")] + \
               [(n, C.c_int) for n in ("down_hl", "down_np", "down_step", "up_hl", "up_np", "up_step")]


lib.awm_add_segment_plan.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(SegmentPlan)]


class StreamRatePlan(C.Structure):
    """awm_stream_rate_plan (include/awm_hip.h): the look-ahead of the tile stream at another sample rate"""
    _fields_ = [(n, C.c_uint64) for n in ("limiter_block", "down_ahead", "mix_ahead", "min_tile")] + \
               [(n, C.c_int) for n in ("down_hl", "down_np", "down_step", "up_hl", "up_np", "up_step")]


lib.awm_add_stream_rate_plan.argtypes = [C.c_int, C.POINTER(StreamRatePlan)]
lib.awm_add_stream_create_rate_at.argtypes = [_vp, _vp, C.c_char_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_vp)]
lib.awm_add_stream_create_payloads_rate_at.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_vp)]
lib.awm_add_stream_sample_rate.argtypes = [_vp]
lib.awm_add_stream_sample_rate.restype = C.c_int
lib.awm_debug_resample_span_d.argtypes = [_vp, _vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(C.c_int)]
lib.awm_debug_add_segments_fused_in_use.argtypes = []
lib.awm_debug_add_segments_fused_in_use.restype = C.c_int
lib.awm_debug_alloc_bytes.argtypes = []
lib.awm_debug_alloc_bytes.restype = C.c_ulonglong
lib.awm_debug_payload_tables_d.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp]
lib.awm_debug_key_templates_d.argtypes = [_vp, _vp, C.c_size_t, _vp]
lib.awm_debug_key_payload_tables_d.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp]
lib.awm_get_watermark_batch_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_add_watermark_batch_keys_d.argtypes = [_vp, _vp, C.c_char_p, C.c_size_t, _vp, _vp, _vp, C.c_int]
lib.awm_get_watermark_batch_keys_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_get_watermark_rate_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, _vp]
lib.awm_get_watermark_batch_rate_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_get_watermark_batch_keys_rate_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_debug_clip_slice_values.argtypes = [C.c_int]
lib.awm_debug_clip_slice_values.restype = C.c_size_t
lib.awm_debug_clip_stage_d.argtypes = [_vp, C.c_size_t, _vp, _vp, C.c_int, C.c_int, _vp, _vp]
lib.awm_get_watermark_batch_rates_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, _vp, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_get_watermark_batch_keys_rates_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, _vp, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_debug_clip_stage_rates_d.argtypes = [_vp, C.c_size_t, _vp, _vp, C.c_int, _vp, _vp, _vp]
lib.awm_get_batch_rates_plan.argtypes = [C.c_size_t, _vp, _vp, _vp, _vp]
lib.awm_get_watermark_batch_rates_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, _vp, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_get_watermark_batch_keys_rates_s16_d.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int, _vp, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_debug_clip_stage_rates_s16_d.argtypes = [_vp, C.c_size_t, _vp, _vp, C.c_int, _vp, _vp, _vp]
lib.awm_debug_clip_form_launches.argtypes = [_vp]
lib.awm_debug_clip_form_launches.restype = None
lib.awm_debug_lane_pcm_bytes.argtypes = [_vp]
lib.awm_debug_lane_pcm_bytes.restype = C.c_size_t
lib.awm_decode_chunk_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, _vp]
lib.awm_tab_up_down.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp]
lib.awm_tab_bit_pos.argtypes = [_vp, _vp]
lib.awm_tab_mix_entries.argtypes = [_vp, _vp]
lib.awm_tab_bit_order.argtypes = [_vp, C.c_size_t, _vp]
lib.awm_tab_frame_mod.argtypes = [_vp, C.c_char_p, _vp]
lib.awm_tab_frame_mod_template.argtypes = [_vp, _vp]
lib.awm_tab_sync_bits.argtypes = [_vp, C.c_int, _vp]
lib.awm_tab_window.argtypes = [C.c_size_t, _vp]
lib.awm_tab_synth_window.argtypes = [_vp]
lib.awm_conv_encode.argtypes = [C.c_int, _vp, C.c_size_t, _vp]
lib.awm_test_gen_noise.argtypes = [_vp, C.c_size_t, _vp]


class RawFormat(C.Structure):
    """awm_raw_format: headerless PCM as with --format raw --raw-rate / --raw-channels / --raw-bits / --raw-encoding / --raw-endian"""
    _fields_ = [("n_channels", C.c_int), ("sample_rate", C.c_int), ("bit_depth", C.c_int), ("encoding", C.c_int), ("big_endian", C.c_int)]


lib.awm_add_watermark_file.argtypes = [_vp, _vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(RawFormat), C.POINTER(RawFormat)]
lib.awm_add_stream_watermark_file.argtypes = [_vp, _vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(RawFormat), C.POINTER(RawFormat), C.c_size_t]
lib.awm_add_stream_create_at.argtypes = [_vp, _vp, C.c_char_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_vp)]
lib.awm_debug_sync_db_sliding_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.c_int, C.c_int, _vp]
lib.awm_debug_sync_db_sliding_rows_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, _vp, C.c_longlong, C.c_longlong,
                                                 _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_longlong, _vp, C.c_longlong]
lib.awm_debug_block_plane_ld.argtypes = [_vp]
lib.awm_debug_block_db_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t, C.c_uint32, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t,
                                     _vp, _vp]
lib.awm_debug_soft_bits_planes_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]
lib.awm_get_watermark_file.argtypes = [_vp, _vp, C.c_char_p, C.POINTER(RawFormat), C.c_size_t, _vp]
lib.awm_add_get_watermark_file.argtypes = [_vp, _vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(RawFormat), C.POINTER(RawFormat), C.c_size_t, _vp]
lib.awm_add_stream_create.argtypes = [_vp, _vp, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(_vp)]
lib.awm_add_stream_destroy.argtypes = [_vp]
lib.awm_add_stream_destroy.restype = None
lib.awm_add_stream_input.argtypes = [_vp]
lib.awm_add_stream_input.restype = C.c_void_p
lib.awm_add_stream_push.argtypes = [_vp, C.c_size_t, C.c_int, _vp, _vp]
lib.awm_add_mix_payloads_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int, _vp, C.c_double, C.c_size_t, _vp, _vp, _vp,
                                       C.c_size_t, C.c_size_t]
lib.awm_add_stream_create_payloads_at.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(_vp)]
lib.awm_add_stream_payloads.argtypes = [_vp]
lib.awm_add_stream_payloads.restype = C.c_size_t
lib.awm_add_stream_push_payloads.argtypes = [_vp, C.c_size_t, C.c_int, _vp, _vp]
lib.awm_add_watermark_payloads_file.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_char_p, _vp, C.POINTER(RawFormat), C.POINTER(RawFormat)]
lib.awm_add_stream_watermark_payloads_file.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_char_p, _vp, C.POINTER(RawFormat), C.POINTER(RawFormat),
                                                       C.c_size_t]
lib.awm_debug_set_payloads_file_tile.argtypes = [C.c_int]
lib.awm_debug_set_payloads_file_tile.restype = None


lib.awm_decode_chunks_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_pcm_decode_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp]
lib.awm_pcm_encode_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
lib.awm_plan_chunks.argtypes = [C.c_size_t, C.c_size_t, _vp, _vp, _vp]
lib.awm_merge_patterns.argtypes = [_vp, _vp, _vp, C.c_int, C.c_size_t, _vp]
lib.awm_prof_name.restype = C.c_char_p
lib.awm_set_speed_params.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
lib.awm_set_speed_params.restype = None
lib.awm_resample_ratio_frames.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double]
lib.awm_resample_ratio_frames.restype = C.c_size_t
lib.awm_resample_ratio_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, _vp, C.c_size_t]
lib.awm_detect_speed_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp]
lib.awm_detect_speed_batch_d.argtypes = [_vp, _vp, C.c_int, C.c_size_t, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]
lib.awm_debug_set_speed_batch_bytes.argtypes = [C.c_size_t]
lib.awm_debug_set_speed_batch_bytes.restype = None
lib.awm_debug_speed_batch_bytes.argtypes = []
lib.awm_debug_speed_batch_bytes.restype = C.c_size_t
lib.awm_debug_set_speed_batch.argtypes = [C.c_int]
lib.awm_debug_set_speed_batch.restype = None
lib.awm_speed_batch_plan.argtypes = [C.c_size_t, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_debug_speed_batch_launches.argtypes = [_vp, _vp, _vp, _vp]
lib.awm_debug_speed_batch_launches.restype = None
lib.awm_debug_speed_scan_batch_d.argtypes = [_vp, _vp, C.c_int, C.c_size_t, _vp, _vp, C.c_int, C.c_int, _vp, C.c_double, C.c_double, C.c_int, C.c_int,
                                             _vp, _vp, C.c_size_t, _vp, _vp, _vp]
lib.awm_speed_clip_location_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_int, _vp]
lib.awm_speed_mags_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_size_t, _vp]
lib.awm_var_resample_table.argtypes = [C.c_double, _vp, C.c_size_t, C.POINTER(C.c_int)]
lib.awm_speed_scan_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                 _vp, C.c_int, C.c_size_t, _vp, _vp]


class Params(C.Structure):
    """awm_params (include/awm_hip.h): the reference's Params, process-wide or per context"""
    _fields_ = [("struct_size", C.c_size_t), ("water_delta", C.c_double), ("mix", C.c_int), ("hard", C.c_int), ("strict", C.c_int),
                ("snr", C.c_int), ("payload_size", C.c_int), ("frames_per_bit", C.c_int), ("sync_threshold2", C.c_double),
                ("get_n_best", C.c_int), ("get_chunk_size", C.c_double), ("detect_speed", C.c_int), ("detect_speed_patient", C.c_int),
                ("try_speed", C.c_double), ("test_speed", C.c_double), ("test_cut", C.c_int), ("test_no_sync", C.c_int),
                ("test_no_limiter", C.c_int), ("test_truncate", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib.awm_params_init(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"awm_params has no field {k}")
            setattr(self, k, v)


lib.awm_params_init.argtypes = [C.POINTER(Params)]
lib.awm_params_init.restype = None
lib.awm_set_global_params.argtypes = [C.POINTER(Params)]
lib.awm_ctx_set_params.argtypes = [_vp, C.POINTER(Params)]
lib.awm_ctx_get_params.argtypes = [_vp, C.POINTER(Params)]
lib.awm_ctx_snr_begin.argtypes = [_vp]
lib.awm_ctx_snr_end.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
lib.awm_get_watermark_keys_d.argtypes = [_vp, _vp, C.c_int, _vp, C.c_size_t, C.c_int, C.c_size_t, _vp, _vp]
lib.awm_get_watermark_keys_file.argtypes = [_vp, _vp, C.c_int, C.c_char_p, C.POINTER(RawFormat), C.c_size_t, _vp, _vp]
# whole streams resident as signed 16-bit PCM: the twins' argument lists
lib.awm_get_watermark_s16_d.argtypes = lib.awm_get_watermark_d.argtypes
lib.awm_get_watermark_keys_s16_d.argtypes = lib.awm_get_watermark_keys_d.argtypes
lib.awm_get_watermark_rate_s16_d.argtypes = lib.awm_get_watermark_rate_d.argtypes
lib.awm_sync_fft_s16_d.argtypes = lib.awm_sync_fft_d.argtypes
lib.awm_sync_search_s16_d.argtypes = lib.awm_sync_search_d.argtypes
lib.awm_block_soft_bits_s16_d.argtypes = lib.awm_block_soft_bits_d.argtypes
lib.awm_debug_sync_db_sliding_rows_s16_d.argtypes = lib.awm_debug_sync_db_sliding_rows_d.argtypes
# whole streams from and to signed 16-bit PCM (`add`, and "watermark, then verify")
lib.awm_add_mix_s16_d.argtypes = lib.awm_add_mix_d.argtypes
lib.awm_add_limit_s16_d.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, _vp, C.c_size_t, C.c_size_t]
lib.awm_add_watermark_s16_d.argtypes = lib.awm_add_watermark_d.argtypes
lib.awm_add_get_watermark_s16_d.argtypes = lib.awm_add_get_watermark_d.argtypes
lib.awm_debug_add_s16_fused_in_use.argtypes = []
lib.awm_debug_lane_add_mix_bytes.argtypes = [_vp]
lib.awm_debug_lane_add_mix_bytes.restype = C.c_size_t


def set_global_params(**kw):
    """the process-wide parameter set from the reference's defaults + the given fields (awm_set_global_params)"""
    p = Params(**kw)
    _check(lib.awm_set_global_params(C.byref(p)), "awm_set_global_params")


def _check(rc, what):
    if rc < 0:
        raise AwmError(f"{what} failed (rc={rc}): {lib.awm_last_error().decode(errors='replace')}")
    return rc


def key_bytes(key=None):
    """16-byte AES key: None -> the all-zero default key, bytes/hex -> as given."""
    if key is None:
        return bytes(16)
    if isinstance(key, str):
        key = bytes.fromhex(key)
    key = bytes(key)
    if len(key) != 16:
        raise ValueError("key must be 16 bytes")
    return key


def test_key(n):
    """Key::set_test_key (reference random.cc:204-209): big-endian u64 in the first 8 bytes."""
    return int(n).to_bytes(8, "big") + bytes(8)


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def set_params(water_delta=0.01, mix=True, frames_per_bit=2, test_no_limiter=False, sync_threshold2=0.35, n_best=8,
               chunk_size_min=30.0):
    lib.awm_set_params(water_delta, int(mix), frames_per_bit, int(test_no_limiter), sync_threshold2, n_best,
                       chunk_size_min)


def set_speed_params(detect_speed=False, patient=False, try_speed=-1.0, test_speed=-1.0):
    """--detect-speed / --detect-speed-patient / --try-speed / --test-speed of `get` (reference wmcommon.hh:49-52)."""
    lib.awm_set_speed_params(int(detect_speed), int(patient), float(try_speed), float(test_speed))


def set_speed_batch_bytes(n_bytes=0):
    """awm_debug_set_speed_batch_bytes: scratch budget of a sub-group of the batched speed search (0: the default)"""
    lib.awm_debug_set_speed_batch_bytes(int(n_bytes))


def speed_batch_bytes():
    """awm_debug_speed_batch_bytes: the scratch budget of a sub-group in force"""
    return int(lib.awm_debug_speed_batch_bytes())


def set_speed_batch(mode=0):
    """awm_debug_set_speed_batch, the clip batches under a speed parameter: 0 (the default) every clip over the lanes with the one-clip
    search; 1 the searches of the short clips as a batch; 2 one clip after the other on the context's lane (the measurement's baseline)"""
    lib.awm_debug_set_speed_batch(int(mode))


def speed_batch_plan(n_frames, n_channels=2, rate=44100, patient=False, budget_bytes=0):
    """awm_speed_batch_plan (no GPU needed): (sub-group of every clip, -1 = under 0.25 s; bytes of every sub-group's first pass)"""
    n = len(n_frames)
    frames = (C.c_size_t * max(n, 1))(*[int(f) for f in n_frames])
    group, nbytes = (C.c_int * max(n, 1))(), (C.c_size_t * max(n, 1))()
    g = _check(lib.awm_speed_batch_plan(n, frames, n_channels, rate, int(patient), int(budget_bytes), group, nbytes), "awm_speed_batch_plan")
    return [int(group[i]) for i in range(n)], [int(nbytes[i]) for i in range(g)]


def speed_batch_launches():
    """awm_debug_speed_batch_launches: launches of the batch forms of (K12, K13, K14, K15) in this process so far"""
    k = [C.c_int(0) for _ in range(4)]
    lib.awm_debug_speed_batch_launches(*[C.byref(x) for x in k])
    return tuple(x.value for x in k)


def plan_chunks(n_frames):
    """WavChunkLoader chunking (host only): list of (first_frame, n_frames, time_offset_seconds)."""
    mx = 4096
    a = np.zeros(mx, np.uint64)
    b = np.zeros(mx, np.uint64)
    t = np.zeros(mx, np.float64)
    n = lib.awm_plan_chunks(n_frames, mx, _np(a), _np(b), _np(t))
    return [(int(a[i]), int(b[i]), float(t[i])) for i in range(n)]


def _pattern_from_dict(d):
    p = Pattern()
    p.time = d["time"]
    p.sync_index = d["sync_index"]
    p.sync_quality = d["sync_quality"]
    p.block_type = d["block_type"]
    p.type = d["type"]
    p.decode_error = d["decode_error"]
    p.speed = d["speed"]
    bits = []
    for ch in d["bits"]:
        v = int(ch, 16)
        bits += [(v >> 3) & 1, (v >> 2) & 1, (v >> 1) & 1, v & 1]
    p.n_bits = len(bits)
    for i, b in enumerate(bits):
        p.bits[i] = b
    return p


PATTERN_DTYPE = np.dtype(Pattern)


def patterns_from_dicts(dicts):
    """pattern dicts -> structured array (PATTERN_DTYPE)"""
    out = np.zeros(len(dicts), PATTERN_DTYPE)
    for i, d in enumerate(dicts):
        p = _pattern_from_dict(d)
        out[i] = np.frombuffer(bytes(p), PATTERN_DTYPE)[0]
    return out


def merge_patterns_raw(key, per_chunk_arrays):
    """ResultSet.merge + sort over per-chunk structured arrays (dtype PATTERN_DTYPE, times already offset); returns dicts.
    No per-pattern Python work: this runs inside the timed region of the multi-GPU path."""
    counts = np.array([len(a) for a in per_chunk_arrays], np.int32)
    total = int(counts.sum())
    if total == 0:
        return []
    arr = np.ascontiguousarray(np.concatenate([a for a in per_chunk_arrays if len(a)]))
    out = np.zeros(total, PATTERN_DTYPE)
    n = lib.awm_merge_patterns(key_bytes(key), arr.ctypes.data_as(C.c_void_p), _np(counts), len(per_chunk_arrays), total,
                               out.ctypes.data_as(C.c_void_p))
    return patterns_to_dicts(out, min(n, total))


def merge_patterns(key, per_chunk):
    """ResultSet.merge + sort over per-chunk pattern lists (times already offset), host only."""
    flat = [_pattern_from_dict(d) for chunk in per_chunk for d in chunk]
    counts = np.array([len(c) for c in per_chunk], np.int32)
    arr = (Pattern * max(1, len(flat)))(*flat)
    mx = max(1, len(flat))
    out = (Pattern * mx)()
    n = lib.awm_merge_patterns(key_bytes(key), C.cast(arr, C.c_void_p), _np(counts), len(per_chunk), mx, C.cast(out, C.c_void_p))
    return [out[i].as_dict() for i in range(min(n, mx))]


# ---- key-derived tables (host only) ---------------------------------------------------------
def tab_up_down(key, stream, frame):
    up = np.zeros(30, np.int32)
    down = np.zeros(30, np.int32)
    lib.awm_tab_up_down(key_bytes(key), stream, frame, _np(up), _np(down))
    return up, down


def tab_bit_pos(key):
    pos = np.zeros(BLOCK_FRAMES, np.int32)
    lib.awm_tab_bit_pos(key_bytes(key), _np(pos))
    return pos


def tab_mix_entries(key):
    out = np.zeros((51480, 3), np.int32)
    n = lib.awm_tab_mix_entries(key_bytes(key), _np(out))
    return out[:n]


def tab_bit_order(key, n):
    out = np.zeros(n, np.uint32)
    lib.awm_tab_bit_order(key_bytes(key), n, _np(out))
    return out


def tab_frame_mod(key, payload_hex):
    out = np.zeros((2, BLOCK_FRAMES, N_BANDS), np.int8)
    _check(lib.awm_tab_frame_mod(key_bytes(key), payload_hex.encode(), _np(out)), "awm_tab_frame_mod")
    return out


def frame_mod_template(key, block_frames=None):
    """awm_tab_frame_mod_template: what of tab_frame_mod depends on the key alone, int16 [2 (A, B)][block frames][81]: 0 KEEP, 1 UP, 2 DOWN,
    or 4 + 2 k + s -- UP if bit k of conv_encode(block type, payload) xor s, else DOWN.  block_frames: 510 + 858 * frames_per_bit as in
    force (default: BLOCK_FRAMES, two frames per bit)."""
    entries = _check(lib.awm_tab_frame_mod_template(key_bytes(key), None), "awm_tab_frame_mod_template")     # (the size in force: nothing written)
    if block_frames is not None and 2 * block_frames * N_BANDS != entries:
        raise ValueError("frame_mod_template: block_frames does not match the parameters in force")
    out = np.zeros((2, entries // (2 * N_BANDS), N_BANDS), np.int16)
    n = _check(lib.awm_tab_frame_mod_template(key_bytes(key), _np(out)), "awm_tab_frame_mod_template")
    assert n == out.size
    return out


def add_segments_fused_in_use():
    """1 if the last add_watermark_segments took the fused path (one launch per stage for the batch)"""
    return lib.awm_debug_add_segments_fused_in_use()


def _add_segments_s16(ctx, name, key_arg, payloads, segments, zero_frames, outs, sample_rate):
    import torch
    payloads, segments, zero_frames = list(payloads), list(segments), list(zero_frames)
    if not (len(payloads) == len(segments) == len(zero_frames)):
        raise ValueError(name + ": payloads, segments and zero_frames must have one length")
    if not segments:
        return []
    per_segment, rates = _segment_rates(sample_rate, len(segments))
    if any(s.dtype != torch.int16 or not s.is_cuda or not s.is_contiguous() for s in segments):
        raise ValueError(name + ": the segments must be contiguous int16 tensors on the device")
    shapes = [(s.shape[0], 1 if s.dim() == 1 else s.shape[1]) for s in segments]
    ch = shapes[0][1]
    if any(s[1] != ch for s in shapes):
        raise ValueError(name + ": the segments must have one channel count")
    if outs is None:
        outs = [torch.empty_like(s) for s in segments]
    elif len(outs) != len(segments) or any(o.shape != s.shape or o.dtype != s.dtype or not o.is_contiguous() for o, s in zip(outs, segments)):
        raise ValueError(name + ": outs must match the segments")
    n = len(segments)
    hexes = (C.c_char_p * n)(*[p.encode() for p in payloads])
    zf = (C.c_size_t * n)(*[int(z) for z in zero_frames])
    src = (C.c_void_p * n)(*[_dev_ptr(s) for s in segments])
    dst = (C.c_void_p * n)(*[_dev_ptr(o) for o in outs])
    frames = (C.c_size_t * n)(*[s[0] for s in shapes])
    if per_segment:
        name = name.replace("_rate_s16_d", "_rates_s16_d")
        _check(getattr(lib, name)(ctx._h, key_arg, n, hexes, zf, src, dst, frames, ch, rates), name)
        return outs
    _check(getattr(lib, name)(ctx._h, key_arg, n, hexes, zf, src, dst, frames, ch, int(sample_rate)), name)
    return outs


def add_watermark_segments_s16(ctx, key, payloads, segments, zero_frames, outs=None, sample_rate=44100):
    """awm_add_watermark_segments_rate_s16_d: Context.add_watermark_segments on segments that are resident as signed 16-bit PCM (int16
    tensors, [frames, channels]), written as 16-bit PCM: outs[i] == pcm_encode(add_watermark_segments(key, ..., pcm_decode(segments[i]), ...),
    16, direct16=True) value for value, without a float copy of a segment and without a launch per segment."""
    return _add_segments_s16(ctx, "awm_add_watermark_segments_rate_s16_d", key_bytes(key), payloads, segments, zero_frames, outs, sample_rate)


def add_watermark_segments_keys_s16(ctx, keys, payloads, segments, zero_frames, outs=None, sample_rate=44100):
    """awm_add_watermark_segments_keys_rate_s16_d: add_watermark_segments_s16 with a key per segment (None, test_key(n) or 16 bytes each)"""
    keys = list(keys)
    if len(keys) != len(list(segments)):
        raise ValueError("awm_add_watermark_segments_keys_rate_s16_d: keys and segments must have one length")
    return _add_segments_s16(ctx, "awm_add_watermark_segments_keys_rate_s16_d", b"".join(key_bytes(k) for k in keys), payloads, segments,
                             zero_frames, outs, sample_rate)


def add_segment_plan(sample_rate, zero_frames, n_frames):
    """awm_add_segment_plan: the window of one stream segment at another sample rate, as a dict of the struct's fields (no GPU needed)"""
    plan = SegmentPlan()
    _check(lib.awm_add_segment_plan(int(sample_rate), int(zero_frames), int(n_frames), C.byref(plan)), "awm_add_segment_plan")
    return {name: int(getattr(plan, name)) for name, _ in SegmentPlan._fields_}


def add_stream_rate_plan(sample_rate):
    """awm_add_stream_rate_plan: the look-ahead and the smallest tile of the tile stream at another sample rate, as a dict (no GPU needed)"""
    plan = StreamRatePlan()
    _check(lib.awm_add_stream_rate_plan(int(sample_rate), C.byref(plan)), "awm_add_stream_rate_plan")
    return {name: int(getattr(plan, name)) for name, _ in StreamRatePlan._fields_}


def _rates_array(sample_rate, n_clips):
    """a sequence of sample rates, one per clip, as a C int array; None for a scalar rate (which keeps meaning one rate for the call)"""
    if isinstance(sample_rate, (int, np.integer)):
        return None
    rates = [int(r) for r in sample_rate]
    if len(rates) != n_clips:
        raise ValueError(f"sample_rate: {len(rates)} rates for {n_clips} clips")
    return (C.c_int * n_clips)(*rates)


def _segment_rates(sample_rate, n_segments):
    """the sample_rate argument of the segment batches -> (a rate per segment?, C int array or None).  An int is one rate for the call; a
    sequence (one rate per segment: ValueError before anything is called otherwise) and None (no array: NULL) take the *_rates_* entry points"""
    if sample_rate is None:
        return True, None
    rates = _rates_array(sample_rate, n_segments)
    return rates is not None, rates


def get_batch_rates_plan(n_frames, sample_rates):
    """awm_get_batch_rates_plan: which way every clip of a batch `get` with a rate per clip goes (0 a group | 1 a lane, fixed-ratio
    resampler | 2 a lane, VResampler | 3 empty) and its length at 44.1 kHz -> (paths, n44), two int64 arrays (no GPU needed).  A rate
    that the batch refuses raises AwmError."""
    n = len(n_frames)
    rates = _rates_array(list(sample_rates), n)
    frames = (C.c_size_t * n)(*[int(f) for f in n_frames])
    paths, n44 = (C.c_int * n)(), (C.c_size_t * n)()
    _check(lib.awm_get_batch_rates_plan(n, frames, rates, paths, n44), "awm_get_batch_rates_plan")
    return np.array(list(paths), np.int64), np.array(list(n44), np.int64)


def tab_sync_bits(key, clip_mode=False):
    rows = 170 if clip_mode else 85
    out = np.zeros((6, rows, 61), np.int32)
    r = lib.awm_tab_sync_bits(key_bytes(key), int(clip_mode), _np(out))
    assert r == rows
    return out


def tab_window(n=1024):
    out = np.zeros(n, np.float32)
    lib.awm_tab_window(n, _np(out))
    return out


def tab_synth_window():
    out = np.zeros(3072, np.float32)
    lib.awm_tab_synth_window(_np(out))
    return out


def var_resample_table(ratio):
    """awm_var_resample_table: the coefficient table resample_ratio uses for `ratio`, [257][hl] float32 (pure host)."""
    hl = C.c_int(0)
    n = lib.awm_var_resample_table(float(ratio), None, 0, C.byref(hl))
    _check(n, "awm_var_resample_table")
    out = np.zeros((257, hl.value), np.float32)
    assert n == out.size
    _check(lib.awm_var_resample_table(float(ratio), _np(out), out.size, C.byref(hl)), "awm_var_resample_table")
    return out


def gen_noise(key, n_values):
    """`audiowmark test-gen-noise` samples (reference audiowmark.cc:399-417): interleaved float32 in [-1, 1)."""
    out = np.zeros(n_values, np.float32)
    lib.awm_test_gen_noise(key_bytes(key), C.c_size_t(n_values), _np(out))
    return out


def conv_encode(block_type, bits):
    bits = np.ascontiguousarray(bits, np.int32)
    out = np.zeros((len(bits) + 15) * 12, np.int32)
    n = lib.awm_conv_encode(block_type, _np(bits), len(bits), _np(out))
    return out[:n]


def _hip_memcpy_dtod(ctx, dst, src, nbytes):
    """device-to-device copy on the context's stream (through torch: the library exports no raw copy)"""
    if nbytes <= 0:
        return
    _as_tensor(dst, nbytes).copy_(_as_tensor(src, nbytes))       # views over raw device pointers; torch's current stream == ctx stream


def _as_tensor(ptr, nbytes, device=None):
    """uint8 VIEW over raw device memory (no copy).  `device`: the torch device the memory lives on (default: the current one) -- a view
    created under another current device would silently become a copy, and bytes received into it would never reach the buffer."""
    import torch

    class _Iface:
        pass
    o = _Iface()
    o.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    t = torch.as_tensor(o, device=device if device is not None else "cuda")
    if nbytes and t.data_ptr() != int(ptr):
        raise AwmError("_as_tensor: torch copied the buffer instead of viewing it (wrong device?)")
    return t


# ---- device side ---------------------------------------------------------------------------
def _dev_ptr(t):
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _out_tensor(out, shape, dtype, device, what):
    """the caller's output buffer of a call that would otherwise allocate one: contiguous, of the call's shape, type and device"""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def _pcm_shape(pcm):
    """(n_frames, n_channels) of an interleaved float32 CUDA tensor shaped [frames, channels] or [frames]."""
    import torch
    assert pcm.dtype == torch.float32 and pcm.is_cuda and pcm.is_contiguous()
    if pcm.dim() == 1:
        return pcm.shape[0], 1
    return pcm.shape[0], pcm.shape[1]


def check_payload_outputs(payloads, pcm, outs):
    """argument check of Context.add_watermark_payloads, before the library is called (needs no GPU): one float32 output of the input's
    shape and device per payload; returns outs as a list (or None)"""
    import torch
    if pcm.dtype != torch.float32 or not pcm.is_contiguous():
        raise ValueError("add_watermark_payloads: pcm must be a contiguous float32 tensor")
    for i, p in enumerate(payloads):
        if not isinstance(p, str):
            raise TypeError(f"add_watermark_payloads: payloads[{i}] must be a hex string")
    if outs is None:
        return None
    outs = list(outs)
    if len(outs) != len(payloads):
        raise ValueError(f"add_watermark_payloads: {len(payloads)} payloads but {len(outs)} outputs")
    for i, o in enumerate(outs):
        if o.dtype != torch.float32 or o.shape != pcm.shape or o.device != pcm.device or not o.is_contiguous():
            raise ValueError(f"add_watermark_payloads: outs[{i}] must be a contiguous float32 tensor of the input's shape and device")
    return outs


def check_payload_paths(payloads, in_path, out_paths):
    """argument check of Context.add_watermark_payloads_file, before the library is called: one output path per payload (hex strings), no
    two of them equal and none equal to the input; returns the output paths as a list of bytes"""
    payloads = list(payloads)
    for i, p in enumerate(payloads):
        if not isinstance(p, str):
            raise TypeError(f"add_watermark_payloads_file: payloads[{i}] must be a hex string")
    if isinstance(out_paths, (str, bytes, os.PathLike)):
        raise TypeError("add_watermark_payloads_file: out_paths must be a list of paths, one per payload")
    outs = [os.fsencode(o) for o in out_paths]
    if len(outs) != len(payloads):
        raise ValueError(f"add_watermark_payloads_file: {len(payloads)} payloads but {len(outs)} output paths")
    seen = {os.path.abspath(os.fsencode(in_path)): -1}
    for i, o in enumerate(outs):
        a = os.path.abspath(o)
        if a in seen:
            other = "the input path" if seen[a] < 0 else f"out_paths[{seen[a]}]"
            raise ValueError(f"add_watermark_payloads_file: out_paths[{i}] equals {other}")
        seen[a] = i
    return outs


def check_mix_payloads(pcm, outs, frame_mods, block_maxes):
    """argument check of Context.add_mix_payloads, before the library is called: one output of the input's shape and one table per payload,
    and either no block maxima or one array per payload"""
    import torch
    outs, frame_mods = list(outs), list(frame_mods)
    if pcm.dtype != torch.float32 or not pcm.is_contiguous():
        raise ValueError("add_mix_payloads: pcm must be a contiguous float32 tensor")
    if len(outs) != len(frame_mods):
        raise ValueError(f"add_mix_payloads: {len(frame_mods)} tables but {len(outs)} outputs")
    for i, o in enumerate(outs):
        if o.dtype != torch.float32 or o.shape != pcm.shape or o.device != pcm.device or not o.is_contiguous():
            raise ValueError(f"add_mix_payloads: outs[{i}] must be a contiguous float32 tensor of the input's shape and device")
    if block_maxes is not None:
        block_maxes = list(block_maxes)
        if len(block_maxes) != len(outs):
            raise ValueError(f"add_mix_payloads: {len(outs)} outputs but {len(block_maxes)} arrays of block maxima")
        if any(b.numel() != block_maxes[0].numel() for b in block_maxes):
            raise ValueError("add_mix_payloads: the arrays of block maxima must have one length")
    return outs, frame_mods, block_maxes


def set_payloads_file_tile(frames1024):
    """(tests, measurements) add_watermark_payloads_file: tile of the fused path in 1024-sample frames (>= 128); 0 (default): automatic"""
    lib.awm_debug_set_payloads_file_tile(int(frames1024))


def set_add_payloads_fused(on):
    """(tests, measurements) add_watermark_payloads: True (default) the fused kernel, False a loop over the single-payload path"""
    lib.awm_debug_set_add_payloads_fused(int(on))


def add_payloads_fused_in_use():
    """1 if the last add_watermark_payloads ran the fused kernel"""
    return lib.awm_debug_add_payloads_fused_in_use()


def set_add_payloads_rate_fused(mode):
    """(tests, measurements) add_watermark_payloads at another sample rate: 2 (default) one down-resample, K2m and K10m where it applies,
    1 one down-resample and K2m, then K10 and K11 per output, 0 a loop over the single-payload path"""
    lib.awm_debug_set_add_payloads_rate_fused(int(mode))


def add_payloads_rate_fused_in_use():
    """which of these paths the last add_watermark_payloads took (0 at 44.1 kHz)"""
    return lib.awm_debug_add_payloads_rate_fused_in_use()


ADD_PAYLOADS_TILE = lib.awm_debug_add_payloads_tile()     # outputs per pass of the fused kernel over the input


class Context:
    """One awm_ctx: a GPU, its stream and workspaces.  Work is enqueued on torch's current stream
    of that device so that torch.cuda events/synchronisation bracket it."""

    def __init__(self, device=0, use_torch_stream=True):
        import torch
        self.device = device
        h = C.c_void_p()
        _check(lib.awm_ctx_create(device, C.byref(h)), "awm_ctx_create")
        self._h = h
        if use_torch_stream:
            s = torch.cuda.current_stream(device)
            _check(lib.awm_ctx_set_stream(self._h, C.c_void_p(s.cuda_stream)), "awm_ctx_set_stream")

    def close(self):
        if self._h:
            lib.awm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib.awm_ctx_synchronize(self._h), "awm_ctx_synchronize")

    # RawConverter::from_raw / to_raw on the device
    def pcm_decode(self, raw_bytes, bit_depth, encoding=0, big_endian=False, out=None):
        import torch
        assert raw_bytes.dtype == torch.uint8 and raw_bytes.is_cuda and raw_bytes.is_contiguous()
        n = raw_bytes.numel() // (bit_depth // 8)
        out = _out_tensor(out, (n,), torch.float32, raw_bytes.device, "pcm_decode")
        _check(lib.awm_pcm_decode_d(self._h, _dev_ptr(raw_bytes), n, bit_depth, encoding, int(big_endian), _dev_ptr(out)), "awm_pcm_decode_d")
        return out

    def pcm_encode(self, samples, bit_depth, encoding=0, big_endian=False, direct16=True, out=None):
        import torch
        assert samples.dtype == torch.float32 and samples.is_cuda and samples.is_contiguous()
        n = samples.numel()
        out = _out_tensor(out, (n * (bit_depth // 8),), torch.uint8, samples.device, "pcm_encode")
        _check(lib.awm_pcm_encode_d(self._h, _dev_ptr(samples), n, bit_depth, encoding, int(big_endian), int(direct16), _dev_ptr(out)),
               "awm_pcm_encode_d")
        return out

    # FFTAnalyzer::fft_range
    def fft_range(self, pcm, start_index, frame_count, hop=1024, out=None):
        import torch
        n, ch = _pcm_shape(pcm)
        out = _out_tensor(out, (frame_count, ch, 513, 2), torch.float32, pcm.device, "fft_range")
        _check(lib.awm_stft_d(self._h, _dev_ptr(pcm), n, ch, start_index, hop, frame_count, _dev_ptr(out)), "awm_stft_d")
        return out

    # add_watermark on resident PCM
    def add_watermark(self, key, payload_hex, pcm, out=None, sample_rate=44100):
        import torch
        n, ch = _pcm_shape(pcm)
        if out is None:
            out = torch.empty_like(pcm)
        _check(lib.awm_add_watermark_d(self._h, key_bytes(key), payload_hex.encode(), _dev_ptr(pcm), _dev_ptr(out), n, ch,
                                       sample_rate), "awm_add_watermark_d")
        return out

    def add_watermark_batch(self, key, payload_hex, clips, outs=None):
        """add_watermark of many independent resident clips (44.1 kHz, same channel count) with one key and payload, dealt to
        the context's work lanes; returns the list of outputs."""
        import torch
        if not clips:
            return []
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        if outs is None:
            outs = [torch.empty_like(c) for c in clips]
        src = (C.c_void_p * len(clips))(*[_dev_ptr(c) for c in clips])
        dst = (C.c_void_p * len(clips))(*[_dev_ptr(o) for o in outs])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        _check(lib.awm_add_watermark_batch_d(self._h, key_bytes(key), payload_hex.encode(), len(clips), src, dst, frames, ch),
               "awm_add_watermark_batch_d")
        return outs

    def add_watermark_segments(self, key, payloads, segments, zero_frames, outs=None, sample_rate=44100):
        """awm_add_watermark_segments_d: a batch of stream segments (resident, at sample_rate, one channel count) with one key, segment i with
        payloads[i] and starting zero_frames[i] samples into its stream; at 44.1 kHz outs[i] == add_watermark_tiles(key, payloads[i],
        segments[i], zero_frames=zero_frames[i]) bit for bit.  Segments may be one tensor many times (one programme, many subscribers).
        Another sample_rate: awm_add_watermark_segments_rate_d; outs[i] == add_watermark(key, payloads[i], zero_frames[i] zeros + segments[i],
        sample_rate)[zero_frames[i]:] bit for bit, computed from a window around the segment.
        sample_rate may be a sequence with one rate per segment (a queue that is not sorted by rate, awm_add_watermark_segments_rates_d):
        outs[i] is bit for bit what the call with segment i alone at sample_rate[i] gives.  The same holds for the three twins below."""
        import torch
        payloads, segments, zero_frames = list(payloads), list(segments), list(zero_frames)
        if not (len(payloads) == len(segments) == len(zero_frames)):
            raise ValueError("add_watermark_segments: payloads, segments and zero_frames must have one length")
        if not segments:
            return []
        per_segment, rates = _segment_rates(sample_rate, len(segments))
        shapes = [_pcm_shape(s) for s in segments]
        ch = shapes[0][1]
        if any(s[1] != ch for s in shapes):
            raise ValueError("add_watermark_segments: the segments must have one channel count")
        if outs is None:
            outs = [torch.empty_like(s) for s in segments]
        elif len(outs) != len(segments) or any(o.shape != s.shape or o.dtype != s.dtype or not o.is_contiguous() for o, s in zip(outs, segments)):
            raise ValueError("add_watermark_segments: outs must match the segments")
        n = len(segments)
        hexes = (C.c_char_p * n)(*[p.encode() for p in payloads])
        zf = (C.c_size_t * n)(*[int(z) for z in zero_frames])
        src = (C.c_void_p * n)(*[_dev_ptr(s) for s in segments])
        dst = (C.c_void_p * n)(*[_dev_ptr(o) for o in outs])
        frames = (C.c_size_t * n)(*[s[0] for s in shapes])
        if per_segment:
            _check(lib.awm_add_watermark_segments_rates_d(self._h, key_bytes(key), n, hexes, zf, src, dst, frames, ch, rates),
                   "awm_add_watermark_segments_rates_d")
            return outs
        if sample_rate != 44100:
            _check(lib.awm_add_watermark_segments_rate_d(self._h, key_bytes(key), n, hexes, zf, src, dst, frames, ch, sample_rate),
                   "awm_add_watermark_segments_rate_d")
            return outs
        _check(lib.awm_add_watermark_segments_d(self._h, key_bytes(key), n, hexes, zf, src, dst, frames, ch), "awm_add_watermark_segments_d")
        return outs

    def add_watermark_segments_keys(self, keys, payloads, segments, zero_frames, outs=None, sample_rate=44100):
        """awm_add_watermark_segments_keys_d / _rate_d: add_watermark_segments with a key per segment (None, test_key(n) or 16 bytes each);
        outs[i] == add_watermark_segments(keys[i], [payloads[i]], [segments[i]], [zero_frames[i]], sample_rate=sample_rate)[0] bit for bit."""
        import torch
        keys, payloads, segments, zero_frames = list(keys), list(payloads), list(segments), list(zero_frames)
        if not (len(keys) == len(payloads) == len(segments) == len(zero_frames)):
            raise ValueError("add_watermark_segments_keys: keys, payloads, segments and zero_frames must have one length")
        if not segments:
            return []
        per_segment, rates = _segment_rates(sample_rate, len(segments))
        shapes = [_pcm_shape(s) for s in segments]
        ch = shapes[0][1]
        if any(s[1] != ch for s in shapes):
            raise ValueError("add_watermark_segments_keys: the segments must have one channel count")
        if outs is None:
            outs = [torch.empty_like(s) for s in segments]
        elif len(outs) != len(segments) or any(o.shape != s.shape or o.dtype != s.dtype or not o.is_contiguous() for o, s in zip(outs, segments)):
            raise ValueError("add_watermark_segments_keys: outs must match the segments")
        n = len(segments)
        kb = b"".join(key_bytes(k) for k in keys)
        hexes = (C.c_char_p * n)(*[p.encode() for p in payloads])
        zf = (C.c_size_t * n)(*[int(z) for z in zero_frames])
        src = (C.c_void_p * n)(*[_dev_ptr(s) for s in segments])
        dst = (C.c_void_p * n)(*[_dev_ptr(o) for o in outs])
        frames = (C.c_size_t * n)(*[s[0] for s in shapes])
        if per_segment:
            _check(lib.awm_add_watermark_segments_keys_rates_d(self._h, kb, n, hexes, zf, src, dst, frames, ch, rates),
                   "awm_add_watermark_segments_keys_rates_d")
            return outs
        if sample_rate != 44100:
            _check(lib.awm_add_watermark_segments_keys_rate_d(self._h, kb, n, hexes, zf, src, dst, frames, ch, sample_rate),
                   "awm_add_watermark_segments_keys_rate_d")
            return outs
        _check(lib.awm_add_watermark_segments_keys_d(self._h, kb, n, hexes, zf, src, dst, frames, ch), "awm_add_watermark_segments_keys_d")
        return outs

    def add_watermark_segments_s16(self, key, payloads, segments, zero_frames, outs=None, sample_rate=44100):
        """awm_add_watermark_segments_rate_s16_d (binding.add_watermark_segments_s16): int16 segments in, int16 segments out"""
        return add_watermark_segments_s16(self, key, payloads, segments, zero_frames, outs, sample_rate)

    def add_watermark_segments_keys_s16(self, keys, payloads, segments, zero_frames, outs=None, sample_rate=44100):
        """awm_add_watermark_segments_keys_rate_s16_d (binding.add_watermark_segments_keys_s16): the same with a key per segment"""
        return add_watermark_segments_keys_s16(self, keys, payloads, segments, zero_frames, outs, sample_rate)

    def key_templates(self, keys):
        """K16t alone (awm_debug_key_templates_d): the templates of the keys, built on the device, int16 [len(keys)][360624]; the first
        2 * 2226 * 81 entries of row i == frame_mod_template(keys[i]), zeros behind.  The default geometry only (AwmError otherwise)."""
        keys = list(keys)
        stride = (2 * BLOCK_FRAMES * N_BANDS + 15) // 16 * 16
        out = np.full((len(keys), stride), -1, np.int16)
        _check(lib.awm_debug_key_templates_d(self._h, b"".join(key_bytes(k) for k in keys), len(keys), _np(out)), "awm_debug_key_templates_d")
        return out

    def key_payload_tables(self, keys, payloads):
        """K16t + K16p (awm_debug_key_payload_tables_d): the frame_mod tables of (keys[i], payloads[i]), built on the device, int8
        [n][2][2226][81]; == tab_frame_mod(keys[i], payloads[i]).  The default geometry only (AwmError otherwise)."""
        keys, payloads = list(keys), list(payloads)
        if len(keys) != len(payloads):
            raise ValueError("key_payload_tables: keys and payloads must have one length")
        hexes = (C.c_char_p * len(payloads))(*[p.encode() for p in payloads])
        out = np.full((len(payloads), 2, BLOCK_FRAMES, N_BANDS), -1, np.int8)
        _check(lib.awm_debug_key_payload_tables_d(self._h, b"".join(key_bytes(k) for k in keys), hexes, len(payloads), _np(out)),
               "awm_debug_key_payload_tables_d")
        return out

    def payload_tables(self, key, payloads, block_frames=None):
        """K16p alone (awm_debug_payload_tables_d): the frame_mod tables of the payloads, built on the device; == tab_frame_mod per payload"""
        payloads = list(payloads)
        hexes = (C.c_char_p * len(payloads))(*[p.encode() for p in payloads])
        in_force = 510 + 858 * self.get_params().frames_per_bit          # (mark_block_frame_count: the library writes that many rows)
        if block_frames is not None and block_frames != in_force:
            raise ValueError("payload_tables: block_frames does not match the context's parameters")
        out = np.zeros((len(payloads), 2, in_force, N_BANDS), np.int8)
        _check(lib.awm_debug_payload_tables_d(self._h, key_bytes(key), hexes, len(payloads), _np(out)), "awm_debug_payload_tables_d")
        return out

    def add_watermark_payloads(self, key, payloads, pcm, outs=None, sample_rate=44100):
        """add_watermark of ONE resident input with many payloads and one key (awm_add_watermark_payloads_d): the input is read and
        transformed once per tile of ADD_PAYLOADS_TILE outputs; returns the list of outputs, outs[p] == add_watermark(key, payloads[p], pcm)."""
        import torch
        payloads = list(payloads)
        outs = check_payload_outputs(payloads, pcm, outs)
        n, ch = _pcm_shape(pcm)
        if outs is None:
            outs = [torch.empty_like(pcm) for _ in payloads]
        if not payloads:
            return []
        hexes = (C.c_char_p * len(payloads))(*[p.encode() for p in payloads])
        dst = (C.c_void_p * len(payloads))(*[_dev_ptr(o) for o in outs])
        _check(lib.awm_add_watermark_payloads_d(self._h, key_bytes(key), hexes, len(payloads), _dev_ptr(pcm), dst, n, ch, sample_rate),
               "awm_add_watermark_payloads_d")
        return outs

    def add_watermark_batch_keys(self, keys, payload_hex, clips, outs=None):
        """the same with ONE KEY PER CLIP (awm_add_watermark_batch_keys_d; BASELINE configs[4]: `--test-key k` for clip k)"""
        import torch
        if not clips:
            return []
        assert len(keys) == len(clips)
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        if outs is None:
            outs = [torch.empty_like(c) for c in clips]
        src = (C.c_void_p * len(clips))(*[_dev_ptr(c) for c in clips])
        dst = (C.c_void_p * len(clips))(*[_dev_ptr(o) for o in outs])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        flat = b"".join(key_bytes(k) for k in keys)
        _check(lib.awm_add_watermark_batch_keys_d(self._h, flat, payload_hex.encode(), len(clips), src, dst, frames, ch),
               "awm_add_watermark_batch_keys_d")
        return outs

    def get_watermark_batch_keys(self, keys, clips, n_threads=0, max_out_per_clip=64, sample_rate=44100):
        """get_watermark of many independent resident clips, clip i with keys[i] alone (awm_get_watermark_batch_keys_d; at another
        sample rate awm_get_watermark_batch_keys_rate_d; sample_rate a sequence, one rate per clip: awm_get_watermark_batch_keys_rates_d)"""
        if not clips:
            return []
        assert len(keys) == len(clips)
        rates = _rates_array(sample_rate, len(clips))
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        ptrs = (C.c_void_p * len(clips))(*[_dev_ptr(c) for c in clips])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        n_out = (C.c_int * len(clips))()
        flat = b"".join(key_bytes(k) for k in keys)
        while True:
            buf = self._pattern_buffer(len(clips) * max_out_per_clip)
            if rates is not None:
                _check(lib.awm_get_watermark_batch_keys_rates_d(self._h, flat, len(clips), ptrs, frames, ch, rates, n_threads,
                                                                max_out_per_clip, C.cast(buf, C.c_void_p), n_out),
                       "awm_get_watermark_batch_keys_rates_d")
            elif sample_rate != 44100:
                _check(lib.awm_get_watermark_batch_keys_rate_d(self._h, flat, len(clips), ptrs, frames, ch, sample_rate, n_threads,
                                                               max_out_per_clip, C.cast(buf, C.c_void_p), n_out),
                       "awm_get_watermark_batch_keys_rate_d")
            else:
                _check(lib.awm_get_watermark_batch_keys_d(self._h, flat, len(clips), ptrs, frames, ch, n_threads, max_out_per_clip,
                                                          C.cast(buf, C.c_void_p), n_out), "awm_get_watermark_batch_keys_d")
            most = max(n_out)
            if most <= max_out_per_clip:
                return [patterns_to_dicts(buf, n_out[i], i * max_out_per_clip) for i in range(len(clips))]
            max_out_per_clip = most

    # ---- file level: the reference's add_watermark / get_watermark (wmcommon.hh:226-228) ----
    def add_watermark_file(self, key, payload_hex, in_path, out_path, raw_in=None, raw_out=None, zero_frames=None):
        """infile -> outfile; raw_* = RawFormat for headerless PCM, None for WAV; zero_frames: add_stream_watermark's start offset"""
        if zero_frames is not None:
            _check(lib.awm_add_stream_watermark_file(self._h, key_bytes(key), payload_hex.encode(), os.fsencode(in_path), os.fsencode(out_path),
                                                     C.byref(raw_in) if raw_in is not None else None,
                                                     C.byref(raw_out) if raw_out is not None else None, zero_frames), "awm_add_stream_watermark_file")
            return
        _check(lib.awm_add_watermark_file(self._h, key_bytes(key), payload_hex.encode(), os.fsencode(in_path), os.fsencode(out_path),
                                          C.byref(raw_in) if raw_in is not None else None,
                                          C.byref(raw_out) if raw_out is not None else None), "awm_add_watermark_file")

    def add_watermark_payloads_file(self, key, payloads, in_path, out_paths, raw_in=None, raw_out=None, zero_frames=None):
        """awm_add_watermark_payloads_file: ONE infile -> out_paths[p] with payloads[p]; every output is the file add_watermark_file writes
        for that payload, the input is read, uploaded and decoded once (44.1 kHz)"""
        payloads = list(payloads)
        outs = check_payload_paths(payloads, in_path, out_paths)
        hexes = (C.c_char_p * len(payloads))(*[p.encode() for p in payloads])
        paths = (C.c_char_p * len(payloads))(*outs)
        rin = C.byref(raw_in) if raw_in is not None else None
        rout = C.byref(raw_out) if raw_out is not None else None
        if zero_frames is not None:
            _check(lib.awm_add_stream_watermark_payloads_file(self._h, key_bytes(key), hexes, len(payloads), os.fsencode(in_path), paths, rin, rout,
                                                              zero_frames), "awm_add_stream_watermark_payloads_file")
            return
        _check(lib.awm_add_watermark_payloads_file(self._h, key_bytes(key), hexes, len(payloads), os.fsencode(in_path), paths, rin, rout),
               "awm_add_watermark_payloads_file")

    def add_get_watermark_file(self, key, payload_hex, in_path, out_path, raw_in=None, raw_out=None):
        """awm_add_get_watermark_file: infile -> outfile, and the pattern list of `get` on what was written (never read back)"""
        return self._patterns(lib.awm_add_get_watermark_file, "awm_add_get_watermark_file", self._h, key_bytes(key), payload_hex.encode(),
                              os.fsencode(in_path), os.fsencode(out_path), C.byref(raw_in) if raw_in is not None else None,
                              C.byref(raw_out) if raw_out is not None else None)

    def get_watermark_file(self, key, in_path, raw_in=None):
        return self._patterns(lib.awm_get_watermark_file, "awm_get_watermark_file", self._h, key_bytes(key), os.fsencode(in_path),
                              C.byref(raw_in) if raw_in is not None else None)

    def sync_db_sliding(self, pcm, bases, count, ld=72):
        """K4s alone (awm_debug_sync_db_sliding_d): dB [stream][81][ld] of `count` windows advancing by 8 samples from every base"""
        import torch
        n, ch = _pcm_shape(pcm)
        b = torch.as_tensor(bases, dtype=torch.int64, device=pcm.device).contiguous()
        out = torch.zeros((b.numel(), 81, ld), dtype=torch.float32, device=pcm.device)
        _check(lib.awm_debug_sync_db_sliding_d(self._h, _dev_ptr(pcm), n, ch, C.c_void_p(b.data_ptr()), b.numel(), count, ld, _dev_ptr(out)),
               "awm_debug_sync_db_sliding_d")
        self.synchronize()
        return out

    def sync_db_sliding_rows(self, pcm, n_frames, bases, counts, count0, rows_per_plane, row_perm, band_pos, first, last, out, have,
                             tail=None, stream_range=None, range_index=None, range_div=1, tables_per_slice=0):
        """K4s alone as the refinement launches it (awm_debug_sync_db_sliding_rows_d): the gathered layout, every table and every buffer the
        caller's own CUDA tensor.  pcm [>= n_frames][channels] float32, bases int64 / counts int32 [n_streams], row_perm int32 and band_pos
        uint8 [slices][rows_per_plane]([81]), out float32 [slots][60][ld], have int8 [slots][stride], tail float32 [slots][stride] or None,
        stream_range int64 [slices][2] and range_index int32 or None.  Writes out / have / tail in place."""
        import torch
        n, ch = _pcm_shape(pcm)
        assert 0 <= n_frames <= n
        want = ((bases, torch.int64, 1), (counts, torch.int32, 1), (row_perm, torch.int32, 0), (band_pos, torch.uint8, 0), (out, torch.float32, 3),
                (have, torch.int8, 2), (tail, torch.float32, 2), (stream_range, torch.int64, 2), (range_index, torch.int32, 1))
        for t, dtype, dim in want:
            assert t is None or (t.dtype == dtype and t.is_cuda and t.is_contiguous() and (not dim or t.dim() == dim))
        assert bases.numel() == counts.numel() and out.shape[1] == 60 and out.shape[0] == have.shape[0] and (tail is None or tail.shape[0] == out.shape[0])
        opt = lambda t: _dev_ptr(t) if t is not None else None
        _check(lib.awm_debug_sync_db_sliding_rows_d(self._h, _dev_ptr(pcm), n_frames, ch, _dev_ptr(bases), _dev_ptr(counts), bases.numel(), count0,
                                                    rows_per_plane, _dev_ptr(row_perm), _dev_ptr(band_pos), first, last, opt(stream_range),
                                                    opt(range_index), range_div, tables_per_slice, out.shape[2], _dev_ptr(out), opt(tail),
                                                    tail.shape[1] if tail is not None else 0, _dev_ptr(have), have.shape[1]),
               "awm_debug_sync_db_sliding_rows_d")
        self.synchronize()

    def add_watermark_tiles(self, key, payload_hex, pcm, tile_frames1024=128, zero_frames=0, sample_rate=44100):
        """awm_add_stream: `add` as a tile loop over resident PCM (the bounded-memory form the file path uses); returns the
        concatenated output -- bit-identical to add_watermark on the whole stream.  zero_frames: the stream starts that many
        samples into the frame / block grid (add_stream_watermark's zero_frames, reference wmadd.cc:501-526).  sample_rate: another
        rate takes awm_add_stream_create_rate_at, whose tiles are counted at that rate."""
        import torch
        n, ch = _pcm_shape(pcm)
        h = C.c_void_p()
        if sample_rate == 44100:
            _check(lib.awm_add_stream_create_at(self._h, key_bytes(key), payload_hex.encode(), ch, tile_frames1024, zero_frames, C.byref(h)),
                   "awm_add_stream_create_at")
        else:
            _check(lib.awm_add_stream_create_rate_at(self._h, key_bytes(key), payload_hex.encode(), ch, sample_rate, tile_frames1024, zero_frames,
                                                     C.byref(h)), "awm_add_stream_create_rate_at")
        out = torch.empty_like(pcm)
        tile = tile_frames1024 * 1024
        done_p = (C.c_void_p * 3)()
        done_n = (C.c_size_t * 3)()
        pos = written = 0
        esz = pcm.element_size() * ch
        try:
            while True:
                got = min(tile, n - pos)
                last = pos + got >= n
                slot = lib.awm_add_stream_input(h)
                if got:
                    _hip_memcpy_dtod(self, slot, pcm.data_ptr() + pos * esz, got * esz)
                k = _check(lib.awm_add_stream_push(h, got, int(last), done_p, done_n), "awm_add_stream_push")
                for i in range(k):
                    _hip_memcpy_dtod(self, out.data_ptr() + written * esz, done_p[i], done_n[i] * esz)
                    written += done_n[i]
                pos += got
                if last:
                    break
            self.synchronize()
        finally:
            lib.awm_add_stream_destroy(h)
        assert written == n
        return out

    def add_watermark_payloads_tiles(self, key, payloads, pcm, tile_frames1024=128, zero_frames=0, sample_rate=44100):
        """awm_add_stream with P payloads: the tile loop over resident PCM for one input and many payloads; returns the list of
        concatenated outputs, outs[p] == add_watermark_tiles(key, payloads[p], pcm, tile_frames1024, zero_frames) bit for bit.
        sample_rate: another rate takes awm_add_stream_create_payloads_rate_at."""
        import torch
        payloads = list(payloads)
        check_payload_outputs(payloads, pcm, None)
        n, ch = _pcm_shape(pcm)
        P = len(payloads)
        hexes = (C.c_char_p * P)(*[p.encode() for p in payloads])
        h = C.c_void_p()
        if sample_rate == 44100:
            _check(lib.awm_add_stream_create_payloads_at(self._h, key_bytes(key), hexes, P, ch, tile_frames1024, zero_frames, C.byref(h)),
                   "awm_add_stream_create_payloads_at")
        else:
            _check(lib.awm_add_stream_create_payloads_rate_at(self._h, key_bytes(key), hexes, P, ch, sample_rate, tile_frames1024, zero_frames,
                                                              C.byref(h)), "awm_add_stream_create_payloads_rate_at")
        outs = [torch.empty_like(pcm) for _ in payloads]
        tile = tile_frames1024 * 1024
        done_p = (C.c_void_p * (3 * P))()
        done_n = (C.c_size_t * 3)()
        pos = written = 0
        esz = pcm.element_size() * ch
        try:
            assert lib.awm_add_stream_payloads(h) == P
            while True:
                got = min(tile, n - pos)
                last = pos + got >= n
                slot = lib.awm_add_stream_input(h)
                if got:
                    _hip_memcpy_dtod(self, slot, pcm.data_ptr() + pos * esz, got * esz)
                k = _check(lib.awm_add_stream_push_payloads(h, got, int(last), done_p, done_n), "awm_add_stream_push_payloads")
                for i in range(k):
                    for p in range(P):
                        _hip_memcpy_dtod(self, outs[p].data_ptr() + written * esz, done_p[i * P + p], done_n[i] * esz)
                    written += done_n[i]
                pos += got
                if last:
                    break
            self.synchronize()
        finally:
            lib.awm_add_stream_destroy(h)
        assert written == n
        return outs

    def resample_frames(self, n_frames, rate_in, rate_out):
        """frames `resample` delivers for n_frames at rate_in (0: the ratio is not supported)"""
        return lib.awm_resample_frames(self._h, n_frames, rate_in, rate_out)

    def resample(self, pcm, rate_in, rate_out, out=None):
        """The stream the reference's loader hands to the decoder for a file at rate_in (zita-resampler restated)."""
        import torch
        n, ch = _pcm_shape(pcm)
        m = lib.awm_resample_frames(self._h, n, rate_in, rate_out)
        if n and not m:
            raise AwmError("resampling %d -> %d Hz is not supported: %s" % (rate_in, rate_out, lib.awm_last_error().decode()))
        out = _out_tensor(out, (m, ch), torch.float32, pcm.device, "resample")
        _check(lib.awm_resample_d(self._h, _dev_ptr(pcm), n, ch, rate_in, rate_out, _dev_ptr(out), m), "awm_resample_d")
        return out

    def resample_span(self, resident, in0, out0, n_out, rate_in, rate_out, out=None):
        """awm_debug_resample_span_d: outputs out0 .. out0 + n_out - 1 of `resample` from the frames in0 .. in0 + len (resident) - 1 of the
        stream (everything else reads as zero) -> (out, 1 if the phase-per-thread kernel ran else 0)"""
        import torch
        n, ch = _pcm_shape(resident)
        out = _out_tensor(out, (n_out, ch) if resident.dim() > 1 else (n_out,), torch.float32, resident.device, "resample_span")
        used = C.c_int(-1)
        _check(lib.awm_debug_resample_span_d(self._h, _dev_ptr(resident), n, in0, out0, n_out, ch, rate_in, rate_out, _dev_ptr(out), C.byref(used)),
               "awm_debug_resample_span_d")
        return out, used.value

    def resample_ratio_frames(self, n_frames, n_channels, ratio, rate=44100, max_in_seconds=-1.0):
        return lib.awm_resample_ratio_frames(n_frames, n_channels, rate, ratio, max_in_seconds)

    def resample_ratio(self, pcm, ratio, rate=44100, max_in_seconds=-1.0, out=None):
        """resample_ratio_truncate (reference resample.cc:96-119): zita's VResampler, restated."""
        import torch
        n, ch = _pcm_shape(pcm)
        m = lib.awm_resample_ratio_frames(n, ch, rate, ratio, max_in_seconds)
        out = _out_tensor(out, (m, ch), torch.float32, pcm.device, "resample_ratio")
        _check(lib.awm_resample_ratio_d(self._h, _dev_ptr(pcm), n, ch, rate, ratio, max_in_seconds, _dev_ptr(out), m),
               "awm_resample_ratio_d")
        return out

    def detect_speed(self, key, pcm, patient=False, rate=44100):
        """detect_speed for one key (reference wmspeed.cc:622-781): (speed to try or None, best speed, best quality)."""
        n, ch = _pcm_shape(pcm)
        speed, quality = C.c_double(0), C.c_double(0)
        rc = lib.awm_detect_speed_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, rate, int(patient), C.byref(speed), C.byref(quality))
        if rc < 0:
            _check(rc, "awm_detect_speed_d")
        return (speed.value if rc else None), speed.value, quality.value

    @staticmethod
    def _speed_batch_args(key_or_keys, clips):
        per_clip = isinstance(key_or_keys, (list, tuple))
        if per_clip:
            assert len(key_or_keys) == len(clips)
            keys = b"".join(key_bytes(k) for k in key_or_keys)
        else:
            keys = key_bytes(key_or_keys)
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        ptrs = (C.c_void_p * len(clips))(*[_dev_ptr(c) if c.numel() else None for c in clips])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        return keys, int(per_clip), ptrs, frames, ch

    def detect_speed_batch(self, key_or_keys, clips, patient=False, rate=44100):
        """awm_detect_speed_batch_d: detect_speed for many resident clips (one key, or a list with a key per clip) with the passes of the
        search in lockstep -> one (speed to try or None, best speed, best quality) per clip, equal to detect_speed on that clip; a
        clip on which detect_speed raises has its negative error code in place of the first element."""
        if not clips:
            return []
        keys, per_clip, ptrs, frames, ch = self._speed_batch_args(key_or_keys, clips)
        n = len(clips)
        speed, quality, use = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        _check(lib.awm_detect_speed_batch_d(self._h, keys, per_clip, n, ptrs, frames, ch, rate, int(patient), _np(speed), _np(quality), _np(use)),
               "awm_detect_speed_batch_d")
        return [((int(use[i]) if use[i] < 0 else float(speed[i]) if use[i] else None), float(speed[i]), float(quality[i])) for i in range(n)]

    def speed_scan_batch(self, key_or_keys, clips, clip_locations, seconds, step, n_steps, n_center_steps, speeds, rate=44100):
        """awm_debug_speed_scan_batch_d: speed_scan for many clips in one launch per kernel; speeds[i] = the list of clip i -> one
        (speeds, qualities) per clip"""
        keys, per_clip, ptrs, frames, ch = self._speed_batch_args(key_or_keys, clips)
        n = len(clips)
        loc = np.ascontiguousarray(clip_locations, np.float64)
        counts = np.array([len(s) for s in speeds], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float64) for s in speeds]) if n else [], np.float64)
        cap = max(int(counts.max()) * (2 * n_center_steps + 1) * (2 * n_steps + 1), 1)
        o_s, o_q, n_out = np.zeros((n, cap)), np.zeros((n, cap)), np.zeros(n, np.int32)
        _check(lib.awm_debug_speed_scan_batch_d(self._h, keys, per_clip, n, ptrs, frames, ch, rate, _np(loc), seconds, step, n_steps, n_center_steps,
                                                _np(flat), _np(counts), cap, _np(o_s), _np(o_q), _np(n_out)), "awm_debug_speed_scan_batch_d")
        for c in n_out:
            _check(int(c), "awm_debug_speed_scan_batch_d (a clip)")
        return [(o_s[i, :n_out[i]].copy(), o_q[i, :n_out[i]].copy()) for i in range(n)]

    def speed_clip_location(self, key, pcm, seconds, candidates=5, rate=44100):
        n, ch = _pcm_shape(pcm)
        loc = C.c_double(0)
        _check(lib.awm_speed_clip_location_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, rate, seconds, candidates, C.byref(loc)),
               "awm_speed_clip_location_d")
        return loc.value

    def speed_mags(self, key, pcm, clip_location, center, seconds, rate=44100):
        n, ch = _pcm_shape(pcm)
        max_rows = int(seconds * 22050 / 128) + 8
        out = np.zeros((max_rows, 510, 2), np.float32)
        rows = lib.awm_speed_mags_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, rate, clip_location, center, seconds, max_rows, _np(out))
        if rows < 0:
            _check(rows, "awm_speed_mags_d")
        return out[:rows]

    def speed_scan(self, key, pcm, clip_location, seconds, step, n_steps, n_center_steps, speeds, rate=44100):
        n, ch = _pcm_shape(pcm)
        sp = np.ascontiguousarray(speeds, np.float64)
        cap = len(sp) * (2 * n_center_steps + 1) * (2 * n_steps + 1)
        o_s, o_q = np.zeros(cap), np.zeros(cap)
        cnt = lib.awm_speed_scan_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, rate, clip_location, seconds, step, n_steps,
                                   n_center_steps, _np(sp), len(sp), cap, _np(o_s), _np(o_q))
        if cnt < 0:
            _check(cnt, "awm_speed_scan_d")
        return o_s[:cnt], o_q[:cnt]

    def add_d(self, pcm, frame_mod, water_delta=0.01, use_limiter=True, out=None):
        import torch
        n, ch = _pcm_shape(pcm)
        if out is None:
            out = torch.empty_like(pcm)
        fm = np.ascontiguousarray(frame_mod, np.int8)
        _check(lib.awm_add_d(self._h, _dev_ptr(pcm), _dev_ptr(out), n, ch, _np(fm), water_delta, int(use_limiter)), "awm_add_d")
        return out

    def add_mix(self, pcm, out, frame_mod, water_delta, first_frame, halo_before, halo_after, block_max, first_block=0):
        n, ch = _pcm_shape(pcm)
        fm = np.ascontiguousarray(frame_mod, np.int8)
        _check(lib.awm_add_mix_d(self._h, _dev_ptr(pcm), _dev_ptr(out), n, ch, _np(fm), water_delta, first_frame,
                                 _dev_ptr(halo_before) if halo_before is not None else None,
                                 _dev_ptr(halo_after) if halo_after is not None else None,
                                 _dev_ptr(block_max) if block_max is not None else None, first_block,
                                 block_max.numel() if block_max is not None else 0), "awm_add_mix_d")

    def add_mix_payloads(self, pcm, outs, frame_mods, water_delta, first_frame, halo_before, halo_after, block_maxes, first_block=0):
        """awm_add_mix_payloads_d: add_mix of one span for len(frame_mods) tables in fused passes; outs[p] / block_maxes[p] (None: no
        limiter) receive what add_mix writes with frame_mods[p]"""
        outs, frame_mods, block_maxes = check_mix_payloads(pcm, outs, frame_mods, block_maxes)
        n, ch = _pcm_shape(pcm)
        P = len(outs)
        fms = [np.ascontiguousarray(fm, np.int8) for fm in frame_mods]
        fm_p = (C.c_void_p * P)(*[_np(fm) for fm in fms])
        out_p = (C.c_void_p * P)(*[_dev_ptr(o) for o in outs])
        bm_p = (C.c_void_p * P)(*[_dev_ptr(b) for b in block_maxes]) if block_maxes is not None else None
        _check(lib.awm_add_mix_payloads_d(self._h, _dev_ptr(pcm), out_p, P, n, ch, fm_p, water_delta, first_frame,
                                          _dev_ptr(halo_before) if halo_before is not None else None,
                                          _dev_ptr(halo_after) if halo_after is not None else None,
                                          bm_p, first_block, block_maxes[0].numel() if block_maxes else 0), "awm_add_mix_payloads_d")

    def add_init_block_max(self, block_max):
        _check(lib.awm_add_init_block_max_d(self._h, _dev_ptr(block_max), block_max.numel()), "awm_add_init_block_max_d")

    def add_limit(self, out, first_sample, block_max, first_block=0):
        n, ch = _pcm_shape(out)
        _check(lib.awm_add_limit_d(self._h, _dev_ptr(out), n, ch, first_sample, _dev_ptr(block_max), first_block,
                                   block_max.numel()), "awm_add_limit_d")

    # SyncFinder::sync_fft
    def sync_fft(self, pcm, index, frame_count, want_frames=None, first=0, last=None, out=None):
        """out: (db, have) buffers of the caller instead of fresh ones (every row is written: zeros for the frames that are skipped)"""
        import torch
        n, ch = _pcm_shape(pcm)
        if last is None:
            last = n * ch
        if out is None:
            db = torch.zeros((frame_count, N_BANDS), dtype=torch.float32, device=pcm.device)
            have = torch.zeros(frame_count, dtype=torch.int8, device=pcm.device)
        else:
            db = _out_tensor(out[0], (frame_count, N_BANDS), torch.float32, pcm.device, "sync_fft (db)")
            have = _out_tensor(out[1], (frame_count,), torch.int8, pcm.device, "sync_fft (have)")
        want = None
        if want_frames is not None:
            want = np.ascontiguousarray(want_frames, np.int8)
        _check(lib.awm_sync_fft_d(self._h, _dev_ptr(pcm), n, ch, index, frame_count, _np(want) if want is not None else None,
                                  first, last, _dev_ptr(db), _dev_ptr(have)), "awm_sync_fft_d")
        return db, have

    # SyncFinder::search
    def sync_search(self, key, pcm, clip_mode=False, max_out=4096):
        n, ch = _pcm_shape(pcm)
        while True:
            idx = np.zeros(max_out, np.uint64)
            q = np.zeros(max_out, np.float64)
            bt = np.zeros(max_out, np.int32)
            cnt = _check(lib.awm_sync_search_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, int(clip_mode), max_out, _np(idx),
                                               _np(q), _np(bt)), "awm_sync_search_d")
            if cnt <= max_out:
                return idx[:cnt], q[:cnt], bt[:cnt]
            max_out = cnt                                    # more scores than the buffer holds: repeat, never truncate

    def search_approx(self, key, pcm, clip_mode=False):
        n, ch = _pcm_shape(pcm)
        max_out = 4 * (n // 1024 + 1)
        idx = np.zeros(max_out, np.uint64)
        raw = np.zeros(max_out, np.float64)
        mean = np.zeros(max_out, np.float64)
        cnt = _check(lib.awm_search_approx_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, int(clip_mode), max_out, _np(idx),
                                             _np(raw), _np(mean)), "awm_search_approx_d")
        return idx[:cnt], raw[:cnt], mean[:cnt]

    # fft_range + mix_decode
    def block_soft_bits(self, key, pcm, indices):
        n, ch = _pcm_shape(pcm)
        idx = np.ascontiguousarray(indices, np.uint64)
        out = np.zeros((len(idx), SOFT_BITS), np.float32)
        ok = np.zeros(len(idx), np.int32)
        _check(lib.awm_block_soft_bits_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, _np(idx), len(idx), _np(out), _np(ok)),
               "awm_block_soft_bits_d")
        return out, ok

    def block_plane_ld(self):
        """row length of the block decoder's dB planes under the parameters in force"""
        return _check(lib.awm_debug_block_plane_ld(self._h), "awm_debug_block_plane_ld")

    def debug_block_db(self, key, pcm, indices, fill=0x7FC00000, slice_range=None, slice_frames=0, planes=None):
        """awm_debug_block_db_d: K4b and K7 as block_soft_bits launches them -> (planes [blocks][channels][81][ld] float32 on the device
        with the cells K4b left alone holding the bit pattern `fill`, soft [blocks][858], slot [blocks]: the row of planes / soft
        of block i, -1 if it runs past the samples).  slice_range: int64 [n_slices][2] on the device, with slice_frames the padded-clip
        mode.  planes: the caller's buffer instead of a fresh one."""
        import torch
        n, ch = _pcm_shape(pcm)
        idx = np.ascontiguousarray(indices, np.uint64)
        if planes is None:
            planes = torch.empty((len(idx), ch, N_BANDS, self.block_plane_ld()), dtype=torch.float32, device=pcm.device)
        assert planes.dtype == torch.float32 and planes.is_cuda and planes.is_contiguous()
        assert slice_range is None or (slice_range.dtype == torch.int64 and slice_range.is_cuda and slice_range.is_contiguous() and slice_range.dim() == 2
                                       and slice_range.shape[1] == 2)
        soft = np.zeros((len(idx), SOFT_BITS), np.float32)
        slot = np.zeros(len(idx), np.int32)
        _check(lib.awm_debug_block_db_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, _np(idx), len(idx), fill,
                                        _dev_ptr(slice_range) if slice_range is not None else None,
                                        slice_range.shape[0] if slice_range is not None else 0, slice_frames, _dev_ptr(planes), planes.numel(),
                                        _np(soft), _np(slot)), "awm_debug_block_db_d")
        return planes, soft, slot

    def debug_soft_bits_planes(self, key, planes, n_blocks=None, channels=None, block_base=None, slice_range=None, range_index=None):
        """awm_debug_soft_bits_planes_d: K7 alone on planes [blocks][channels][81][ld] float32 of the caller (device) -> soft [blocks][858];
        block_base int64 [blocks], slice_range int64 [n_slices][2], range_index int32 [blocks] (device, all or none): the padded-clip mode"""
        import torch
        assert planes.dtype == torch.float32 and planes.is_cuda and planes.is_contiguous()
        n_blocks = planes.shape[0] if n_blocks is None else n_blocks
        channels = planes.shape[1] if channels is None else channels
        for t, dtype in ((block_base, torch.int64), (slice_range, torch.int64), (range_index, torch.int32)):
            assert t is None or (t.dtype == dtype and t.is_cuda and t.is_contiguous())
        opt = lambda t: _dev_ptr(t) if t is not None else None
        soft = np.zeros((max(n_blocks, 1), SOFT_BITS), np.float32)
        _check(lib.awm_debug_soft_bits_planes_d(self._h, key_bytes(key), _dev_ptr(planes), planes.numel(), n_blocks, channels, opt(block_base),
                                                opt(slice_range), opt(range_index), slice_range.shape[0] if slice_range is not None else 0,
                                                _np(soft)), "awm_debug_soft_bits_planes_d")
        return soft[:n_blocks]

    # conv_decode_soft
    def viterbi_decode(self, block_type, soft):
        soft = np.ascontiguousarray(soft, np.float32)
        if soft.ndim == 1:
            soft = soft[None, :]
        n, coded_len = soft.shape
        rate = 12 if block_type == 2 else 6
        bits = np.zeros((n, coded_len // rate - 15), np.int32)
        err = np.zeros(n, np.float32)
        _check(lib.awm_viterbi_decode(self._h, block_type, _np(soft), coded_len, n, _np(bits), _np(err)), "awm_viterbi_decode")
        return bits, err

    def _pattern_buffer(self, max_out):
        # one page-sized ctypes array per context, reused: allocating and zeroing 4096 patterns costs ~0.4 ms per call
        buf = getattr(self, "_pat_buf", None)
        if buf is None or len(buf) < max_out:
            buf = self._pat_buf = (Pattern * max_out)()
        return buf

    def _patterns(self, fn, what, *args, max_out=4096):
        # the C ABI returns the number of patterns FOUND; when that exceeds the buffer the call is repeated with a buffer
        # that holds them all (never a silently truncated list)
        while True:
            buf = self._pattern_buffer(max_out)
            cnt = _check(fn(*args, max_out, C.cast(buf, C.c_void_p)), what)
            if cnt <= max_out:
                return patterns_to_dicts(buf, cnt)
            max_out = cnt

    # get_watermark on resident PCM (chunk loop, BlockDecoder, ClipDecoder, merge, sort)
    def get_watermark(self, key, pcm, sample_rate=44100):
        """sample_rate != 44100 (awm_get_watermark_rate_d): the result of get_watermark on resample (pcm, sample_rate, 44100)"""
        n, ch = _pcm_shape(pcm)
        if sample_rate != 44100:
            return self._patterns(lib.awm_get_watermark_rate_d, "awm_get_watermark_rate_d", self._h, key_bytes(key), _dev_ptr(pcm), n, ch,
                                  sample_rate)
        return self._patterns(lib.awm_get_watermark_d, "awm_get_watermark_d", self._h, key_bytes(key), _dev_ptr(pcm), n, ch)

    def clip_stage(self, clips, sample_rate, out=None):
        """awm_debug_clip_stage_d: stage 0 of one group of 1 .. 64 short clips alone -> (slices [n_clips, slice values] float32 on the
        device, ranges [n_clips, 2] int64: first non-zero value / last + 1 as absolute indices, -1 / 0 for a silent clip).  out: a
        buffer of that shape to write into (what the stage leaves out keeps its contents).  sample_rate a sequence, one rate per clip:
        awm_debug_clip_stage_rates_d."""
        import torch
        rates = _rates_array(sample_rate, len(clips))
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        values = lib.awm_debug_clip_slice_values(ch)
        if out is None:
            out = torch.zeros((len(clips), values), dtype=torch.float32, device=clips[0].device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == len(clips) * values
        ptrs = (C.c_void_p * len(clips))(*[_dev_ptr(c) for c in clips])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        ranges = np.zeros((len(clips), 2), np.int64)
        if rates is not None:
            _check(lib.awm_debug_clip_stage_rates_d(self._h, len(clips), ptrs, frames, ch, rates, _dev_ptr(out), _np(ranges)),
                   "awm_debug_clip_stage_rates_d")
        else:
            _check(lib.awm_debug_clip_stage_d(self._h, len(clips), ptrs, frames, ch, sample_rate, _dev_ptr(out), _np(ranges)),
                   "awm_debug_clip_stage_d")
        return out, ranges

    def add_get_watermark(self, key, payload_hex, pcm, out, sample_rate=44100):
        """awm_add_get_watermark_d: add_watermark into `out`, then get_watermark of `out`, as one call (`get` starts a chunk as soon as
        the limiter has passed it); returns the pattern list -- the results of the two separate calls."""
        n, ch = _pcm_shape(pcm)
        assert _pcm_shape(out) == (n, ch) and out.data_ptr() != pcm.data_ptr()
        return self._patterns(lib.awm_add_get_watermark_d, "awm_add_get_watermark_d", self._h, key_bytes(key), payload_hex.encode(),
                              _dev_ptr(pcm), _dev_ptr(out), n, ch, sample_rate)

    def set_params(self, params=None, **kw):
        """Give this context its own parameter set (awm_ctx_set_params): a Params object, or the fields that differ from what is
        in force now as keywords; set_params() without anything returns the context to the process-wide set."""
        if params is None and kw:
            params = self.get_params()
            for k, v in kw.items():
                if k not in dict(Params._fields_):
                    raise TypeError(f"awm_params has no field {k}")
                setattr(params, k, v)
        _check(lib.awm_ctx_set_params(self._h, C.byref(params) if params is not None else None), "awm_ctx_set_params")

    def get_params(self):
        p = Params()
        _check(lib.awm_ctx_get_params(self._h, C.byref(p)), "awm_ctx_get_params")
        return p

    def snr_begin(self):
        """`add --snr`: every add of this context accumulates input and watermark power (before the limiter) until snr_end"""
        _check(lib.awm_ctx_snr_begin(self._h), "awm_ctx_snr_begin")

    def snr_end(self):
        """-> SNR in dB = 10 log10 (power of the input / power of the watermark signal), reference wmadd.cc:553-563, 591-592"""
        import math
        sig, delta = C.c_double(), C.c_double()
        _check(lib.awm_ctx_snr_end(self._h, C.byref(sig), C.byref(delta)), "awm_ctx_snr_end")
        return 10 * math.log10(sig.value / delta.value) if delta.value > 0 else float("inf")

    def _patterns_keys(self, fn, what, keys, *args, max_out=4096):
        flat = b"".join(key_bytes(k) for k in keys)
        while True:
            buf = self._pattern_buffer(max_out)
            which = (C.c_int * max_out)()
            cnt = _check(fn(self._h, flat, len(keys), *args, max_out, C.cast(buf, C.c_void_p), which), what)
            if cnt <= max_out:
                pats = patterns_to_dicts(buf, cnt)
                for p, k in zip(pats, which):
                    p["key_index"] = int(k)
                return pats
            max_out = cnt

    def get_watermark_keys(self, keys, pcm):
        """get_watermark with the reference's key LIST (`--key a --key b`): one pass over the material, every pattern tells the
        position of its key in the list ("key_index")."""
        n, ch = _pcm_shape(pcm)
        return self._patterns_keys(lib.awm_get_watermark_keys_d, "awm_get_watermark_keys_d", keys, _dev_ptr(pcm), n, ch)

    def get_watermark_keys_file(self, keys, in_path, raw_in=None):
        return self._patterns_keys(lib.awm_get_watermark_keys_file, "awm_get_watermark_keys_file", keys, os.fsencode(in_path),
                                   C.byref(raw_in) if raw_in is not None else None)

    def get_watermark_batch(self, key, clips, n_threads=0, max_out_per_clip=64, sample_rate=44100):
        """get_watermark of many independent resident clips (same channel count), spread over the context's work lanes;
        returns one pattern list per clip.  sample_rate != 44100 (awm_get_watermark_batch_rate_d): every clip is at that rate, its
        result that of the clip resampled to 44.1 kHz.  sample_rate a sequence (awm_get_watermark_batch_rates_d): one rate per clip."""
        if not clips:
            return []
        rates = _rates_array(sample_rate, len(clips))
        shapes = [_pcm_shape(c) for c in clips]
        ch = shapes[0][1]
        assert all(s[1] == ch for s in shapes)
        ptrs = (C.c_void_p * len(clips))(*[_dev_ptr(c) for c in clips])
        frames = (C.c_size_t * len(clips))(*[s[0] for s in shapes])
        n_out = (C.c_int * len(clips))()
        while True:
            buf = self._pattern_buffer(len(clips) * max_out_per_clip)
            if rates is not None:
                _check(lib.awm_get_watermark_batch_rates_d(self._h, key_bytes(key), len(clips), ptrs, frames, ch, rates, n_threads,
                                                           max_out_per_clip, C.cast(buf, C.c_void_p), n_out), "awm_get_watermark_batch_rates_d")
            elif sample_rate != 44100:
                _check(lib.awm_get_watermark_batch_rate_d(self._h, key_bytes(key), len(clips), ptrs, frames, ch, sample_rate, n_threads,
                                                          max_out_per_clip, C.cast(buf, C.c_void_p), n_out), "awm_get_watermark_batch_rate_d")
            else:
                _check(lib.awm_get_watermark_batch_d(self._h, key_bytes(key), len(clips), ptrs, frames, ch, n_threads, max_out_per_clip,
                                                     C.cast(buf, C.c_void_p), n_out), "awm_get_watermark_batch_d")
            most = max(n_out)
            if most <= max_out_per_clip:
                return [patterns_to_dicts(buf, n_out[i], i * max_out_per_clip) for i in range(len(clips))]
            max_out_per_clip = most           # a clip found more patterns than a slot holds: repeat with slots that fit

    # ---- the batches on clips that are resident as signed 16-bit PCM ----
    @staticmethod
    def _s16_clips(clips, sample_rate):
        """(pointers, frames, channels, rates or None) of torch.int16 clips shaped [frames, channels] or [frames]; a scalar rate becomes a rate
        per clip, 44100 the NULL that means "all at 44.1 kHz" """
        import torch
        for c in clips:
            assert c.dtype == torch.int16 and c.is_cuda and c.is_contiguous()
        ch = 1 if clips[0].dim() == 1 else clips[0].shape[1]
        assert all((1 if c.dim() == 1 else c.shape[1]) == ch for c in clips)
        rates = _rates_array(sample_rate, len(clips))
        if rates is None and sample_rate != 44100:
            rates = (C.c_int * len(clips))(*[int(sample_rate)] * len(clips))
        ptrs = (C.c_void_p * len(clips))(*[C.c_void_p(c.data_ptr()) for c in clips])
        frames = (C.c_size_t * len(clips))(*[c.shape[0] for c in clips])
        return ptrs, frames, ch, rates

    def _batch_s16(self, fn, what, key_arg, clips, n_threads, max_out_per_clip, sample_rate):
        if not clips:
            return []
        ptrs, frames, ch, rates = self._s16_clips(clips, sample_rate)
        n_out = (C.c_int * len(clips))()
        while True:
            buf = self._pattern_buffer(len(clips) * max_out_per_clip)
            _check(fn(self._h, key_arg, len(clips), ptrs, frames, ch, rates, n_threads, max_out_per_clip, C.cast(buf, C.c_void_p), n_out), what)
            most = max(n_out)
            if most <= max_out_per_clip:
                return [patterns_to_dicts(buf, n_out[i], i * max_out_per_clip) for i in range(len(clips))]
            max_out_per_clip = most

    def get_watermark_batch_s16(self, key, clips, n_threads=0, max_out_per_clip=64, sample_rate=44100):
        """awm_get_watermark_batch_rates_s16_d: get_watermark_batch on torch.int16 clips (signed 16-bit PCM, interleaved) as they are -- the
        result is that of the float call on pcm_decode of every clip, and a short clip is never copied to float.  sample_rate: one rate
        or a sequence, one rate per clip."""
        return self._batch_s16(lib.awm_get_watermark_batch_rates_s16_d, "awm_get_watermark_batch_rates_s16_d", key_bytes(key), clips, n_threads,
                               max_out_per_clip, sample_rate)

    def get_watermark_batch_keys_s16(self, keys, clips, n_threads=0, max_out_per_clip=64, sample_rate=44100):
        """awm_get_watermark_batch_keys_rates_s16_d: the same with keys[i] for clip i alone"""
        assert len(keys) == len(clips)
        return self._batch_s16(lib.awm_get_watermark_batch_keys_rates_s16_d, "awm_get_watermark_batch_keys_rates_s16_d",
                               b"".join(key_bytes(k) for k in keys), clips, n_threads, max_out_per_clip, sample_rate)

    def clip_stage_s16(self, clips, sample_rate=44100, out=None):
        """awm_debug_clip_stage_rates_s16_d: clip_stage on torch.int16 clips -> (slices, ranges), bit for bit those of clip_stage on the
        decoded clips"""
        import torch
        ptrs, frames, ch, rates = self._s16_clips(clips, sample_rate)
        values = lib.awm_debug_clip_slice_values(ch)
        if out is None:
            out = torch.zeros((len(clips), values), dtype=torch.float32, device=clips[0].device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == len(clips) * values
        ranges = np.zeros((len(clips), 2), np.int64)
        _check(lib.awm_debug_clip_stage_rates_s16_d(self._h, len(clips), ptrs, frames, ch, rates, _dev_ptr(out), _np(ranges)),
               "awm_debug_clip_stage_rates_s16_d")
        return out, ranges

    # ---- whole streams resident as signed 16-bit PCM (awm_get_watermark_s16_d and its twins) ----
    @staticmethod
    def _s16_shape(pcm16):
        """(n_frames, n_channels) of an interleaved torch.int16 CUDA tensor shaped [frames, channels] or [frames]; a view at any even
        address is fine as long as it is contiguous"""
        import torch
        assert pcm16.dtype == torch.int16 and pcm16.is_cuda and pcm16.is_contiguous()
        return (pcm16.shape[0], 1) if pcm16.dim() == 1 else (pcm16.shape[0], pcm16.shape[1])

    def get_watermark_s16(self, key, pcm16, sample_rate=44100):
        """awm_get_watermark_s16_d / awm_get_watermark_rate_s16_d: get_watermark on a torch.int16 stream as it is -- the result is that of
        get_watermark (pcm_decode of the same bytes, sample_rate), and no float copy of the stream is made"""
        n, ch = self._s16_shape(pcm16)
        ptr = C.c_void_p(pcm16.data_ptr())
        if sample_rate != 44100:
            return self._patterns(lib.awm_get_watermark_rate_s16_d, "awm_get_watermark_rate_s16_d", self._h, key_bytes(key), ptr, n, ch, sample_rate)
        return self._patterns(lib.awm_get_watermark_s16_d, "awm_get_watermark_s16_d", self._h, key_bytes(key), ptr, n, ch)

    # ---- whole streams from and to signed 16-bit PCM (awm_add_watermark_s16_d and its twins) ----
    def add_watermark_s16(self, key, payload_hex, pcm16, out=None, sample_rate=44100):
        """awm_add_watermark_s16_d: add_watermark on a torch.int16 stream as it is, into a torch.int16 `out` (None: a fresh tensor; `out` may
        BE pcm16) -- value for value pcm_encode (direct16) of add_watermark (pcm_decode of the same bytes); returns `out`"""
        import torch
        n, ch = self._s16_shape(pcm16)
        if out is None:
            out = torch.empty_like(pcm16)
        assert self._s16_shape(out) == (n, ch)
        _check(lib.awm_add_watermark_s16_d(self._h, key_bytes(key), payload_hex.encode(), C.c_void_p(pcm16.data_ptr()),
                                           C.c_void_p(out.data_ptr()), n, ch, sample_rate), "awm_add_watermark_s16_d")
        return out

    def add_get_watermark_s16(self, key, payload_hex, pcm16, out, sample_rate=44100):
        """awm_add_get_watermark_s16_d: add_watermark_s16 into `out`, then get_watermark_s16 of `out`, as one call; returns the pattern
        list -- the results of the two separate calls"""
        n, ch = self._s16_shape(pcm16)
        assert self._s16_shape(out) == (n, ch)
        return self._patterns(lib.awm_add_get_watermark_s16_d, "awm_add_get_watermark_s16_d", self._h, key_bytes(key), payload_hex.encode(),
                              C.c_void_p(pcm16.data_ptr()), C.c_void_p(out.data_ptr()), n, ch, sample_rate)

    def add_mix_s16(self, pcm16, out, frame_mod, water_delta, first_frame, halo_before, halo_after, block_max, first_block=0):
        """awm_add_mix_s16_d: add_mix on a torch.int16 span (and torch.int16 halos) -- `out` (float32) and block_max are bit for bit those of
        add_mix on the decoded span and halos"""
        n, ch = self._s16_shape(pcm16)
        fm = np.ascontiguousarray(frame_mod, np.int8)
        _check(lib.awm_add_mix_s16_d(self._h, C.c_void_p(pcm16.data_ptr()), _dev_ptr(out), n, ch, _np(fm), water_delta, first_frame,
                                     C.c_void_p(halo_before.data_ptr()) if halo_before is not None else None,
                                     C.c_void_p(halo_after.data_ptr()) if halo_after is not None else None,
                                     _dev_ptr(block_max) if block_max is not None else None, first_block,
                                     block_max.numel() if block_max is not None else 0), "awm_add_mix_s16_d")

    def add_limit_s16(self, mix, out, first_sample, block_max, first_block=0):
        """awm_add_limit_s16_d: the limiter's ramp over the float mix (block_max None: no ramp), encoded into the torch.int16 `out` -- value
        for value pcm_encode (direct16) of what add_limit leaves in a copy of `mix`; `mix` is not modified"""
        n, ch = _pcm_shape(mix)
        assert self._s16_shape(out) == (n, ch)
        _check(lib.awm_add_limit_s16_d(self._h, _dev_ptr(mix), C.c_void_p(out.data_ptr()), n, ch, first_sample,
                                       _dev_ptr(block_max) if block_max is not None else None, first_block,
                                       block_max.numel() if block_max is not None else 0), "awm_add_limit_s16_d")

    def get_watermark_keys_s16(self, keys, pcm16):
        """awm_get_watermark_keys_s16_d: get_watermark_keys on a torch.int16 stream"""
        n, ch = self._s16_shape(pcm16)
        return self._patterns_keys(lib.awm_get_watermark_keys_s16_d, "awm_get_watermark_keys_s16_d", keys, C.c_void_p(pcm16.data_ptr()), n, ch)

    def sync_fft_s16(self, pcm16, index, frame_count, want_frames=None, first=0, last=None, out=None):
        """awm_sync_fft_s16_d: sync_fft on a torch.int16 stream"""
        import torch
        n, ch = self._s16_shape(pcm16)
        if last is None:
            last = n * ch
        if out is None:
            db = torch.zeros((frame_count, N_BANDS), dtype=torch.float32, device=pcm16.device)
            have = torch.zeros(frame_count, dtype=torch.int8, device=pcm16.device)
        else:
            db = _out_tensor(out[0], (frame_count, N_BANDS), torch.float32, pcm16.device, "sync_fft_s16 (db)")
            have = _out_tensor(out[1], (frame_count,), torch.int8, pcm16.device, "sync_fft_s16 (have)")
        want = np.ascontiguousarray(want_frames, np.int8) if want_frames is not None else None
        _check(lib.awm_sync_fft_s16_d(self._h, C.c_void_p(pcm16.data_ptr()), n, ch, index, frame_count, _np(want) if want is not None else None,
                                      first, last, _dev_ptr(db), _dev_ptr(have)), "awm_sync_fft_s16_d")
        return db, have

    def sync_search_s16(self, key, pcm16, clip_mode=False, max_out=4096):
        """awm_sync_search_s16_d: sync_search on a torch.int16 stream"""
        n, ch = self._s16_shape(pcm16)
        while True:
            idx = np.zeros(max_out, np.uint64)
            q = np.zeros(max_out, np.float64)
            bt = np.zeros(max_out, np.int32)
            cnt = _check(lib.awm_sync_search_s16_d(self._h, key_bytes(key), C.c_void_p(pcm16.data_ptr()), n, ch, int(clip_mode), max_out, _np(idx),
                                                   _np(q), _np(bt)), "awm_sync_search_s16_d")
            if cnt <= max_out:
                return idx[:cnt], q[:cnt], bt[:cnt]
            max_out = cnt

    def block_soft_bits_s16(self, key, pcm16, indices):
        """awm_block_soft_bits_s16_d: block_soft_bits on a torch.int16 stream"""
        n, ch = self._s16_shape(pcm16)
        idx = np.ascontiguousarray(indices, np.uint64)
        out = np.zeros((len(idx), SOFT_BITS), np.float32)
        ok = np.zeros(len(idx), np.int32)
        _check(lib.awm_block_soft_bits_s16_d(self._h, key_bytes(key), C.c_void_p(pcm16.data_ptr()), n, ch, _np(idx), len(idx), _np(out), _np(ok)),
               "awm_block_soft_bits_s16_d")
        return out, ok

    def sync_db_sliding_rows_s16(self, pcm16, n_frames, bases, counts, count0, rows_per_plane, row_perm, band_pos, first, last, out, have,
                                 tail=None, stream_range=None, range_index=None, range_div=1, tables_per_slice=0):
        """awm_debug_sync_db_sliding_rows_s16_d: sync_db_sliding_rows on a torch.int16 stream (the default forms only)"""
        import torch
        n, ch = self._s16_shape(pcm16)
        assert 0 <= n_frames <= n
        want = ((bases, torch.int64, 1), (counts, torch.int32, 1), (row_perm, torch.int32, 0), (band_pos, torch.uint8, 0), (out, torch.float32, 3),
                (have, torch.int8, 2), (tail, torch.float32, 2), (stream_range, torch.int64, 2), (range_index, torch.int32, 1))
        for t, dtype, dim in want:
            assert t is None or (t.dtype == dtype and t.is_cuda and t.is_contiguous() and (not dim or t.dim() == dim))
        assert bases.numel() == counts.numel() and out.shape[1] == 60 and out.shape[0] == have.shape[0] and (tail is None or tail.shape[0] == out.shape[0])
        opt = lambda t: _dev_ptr(t) if t is not None else None
        _check(lib.awm_debug_sync_db_sliding_rows_s16_d(self._h, C.c_void_p(pcm16.data_ptr()), n_frames, ch, _dev_ptr(bases), _dev_ptr(counts),
                                                        bases.numel(), count0, rows_per_plane, _dev_ptr(row_perm), _dev_ptr(band_pos), first, last,
                                                        opt(stream_range), opt(range_index), range_div, tables_per_slice, out.shape[2],
                                                        _dev_ptr(out), opt(tail), tail.shape[1] if tail is not None else 0, _dev_ptr(have),
                                                        have.shape[1]), "awm_debug_sync_db_sliding_rows_s16_d")
        self.synchronize()

    def decode_chunks(self, key, pcm, chunks, first_is_stream_start, max_out=8192):
        """decode() of several chunks [(first_frame, n_frames), ...] of one resident buffer; returns one pattern list per
        chunk (times relative to the chunk)."""
        n, ch = _pcm_shape(pcm)
        first = np.array([c[0] for c in chunks], np.uint64)
        count = np.array([c[1] for c in chunks], np.uint64)
        while True:
            buf = self._pattern_buffer(max_out)
            which = np.zeros(max_out, np.int32)
            cnt = _check(lib.awm_decode_chunks_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, len(chunks), _np(first), _np(count),
                                                 int(first_is_stream_start), max_out, C.cast(buf, C.c_void_p), _np(which)),
                         "awm_decode_chunks_d")
            if cnt <= max_out:
                break
            max_out = cnt
        out = [[] for _ in chunks]
        for i, d in enumerate(patterns_to_dicts(buf, cnt)):
            out[which[i]].append(d)
        return out

    def decode_chunks_raw(self, key, pcm, chunks, first_is_stream_start, max_out=8192):
        """decode_chunks without building Python objects: (patterns, which) -- a structured array (PATTERN_DTYPE, times relative
        to the chunk) and the index into `chunks` each pattern belongs to."""
        n, ch = _pcm_shape(pcm)
        first = np.array([c[0] for c in chunks], np.uint64)
        count = np.array([c[1] for c in chunks], np.uint64)
        while True:
            out = np.zeros(max_out, PATTERN_DTYPE)
            which = np.zeros(max_out, np.int32)
            cnt = _check(lib.awm_decode_chunks_d(self._h, key_bytes(key), _dev_ptr(pcm), n, ch, len(chunks), _np(first), _np(count),
                                                 int(first_is_stream_start), max_out, out.ctypes.data_as(C.c_void_p), _np(which)),
                         "awm_decode_chunks_d")
            if cnt <= max_out:
                return out[:cnt], which[:cnt]
            max_out = cnt

    def decode_chunk(self, key, pcm, first_chunk=True):
        n, ch = _pcm_shape(pcm)
        return self._patterns(lib.awm_decode_chunk_d, "awm_decode_chunk_d", self._h, key_bytes(key), _dev_ptr(pcm), n, ch,
                              int(first_chunk))
