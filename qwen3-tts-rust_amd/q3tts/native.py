"""Thin object wrapper over the C ABI (include/q3tts.h). No arithmetic happens in Python."""
import ctypes as C
import math
import os
import weakref

import numpy as np

from . import _abi

f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def _ptr(a, typ):
    return a.ctypes.data_as(typ)


_LANG_DEFAULT = object()


def make_prompt_desc(text_ids, spk_emb=None, lang_id=_LANG_DEFAULT, spk_id=-1, instruct_ids=None, ref_codes=None,
                     ref_text_ids=None, part="whole"):
    """Returns (PromptDesc, keepalive list).

    part: "whole" (default) describes a whole prompt; "voice" only its voice part, for NativeEngine.create_prefix (text_ids must be None or
    empty); "text" only its text part, for a request behind a prefix (every voice field must be left unset; lang_id then defaults to None).
    lang_id defaults to 2055 for "whole" and "voice"."""
    if part not in ("whole", "voice", "text"):
        raise ValueError(f"part must be 'whole', 'voice' or 'text', not {part!r}")
    if part == "voice" and text_ids is not None and len(text_ids) > 0:
        raise ValueError("a voice-only desc has no text: text_ids must be None or empty")
    if part == "text":
        given = [n for n, v in (("spk_emb", spk_emb), ("instruct_ids", instruct_ids), ("ref_codes", ref_codes),
                                ("ref_text_ids", ref_text_ids)) if v is not None]
        if spk_id is not None and spk_id >= 0:
            given.append("spk_id")
        if lang_id is not _LANG_DEFAULT and lang_id is not None and lang_id >= 0:
            given.append("lang_id")
        if given:
            raise ValueError(f"a text-only desc takes its voice from the prefix: {', '.join(given)} must be unset")
        lang_id, spk_id = None, -1
    elif lang_id is _LANG_DEFAULT:
        lang_id = 2055
    keep = []
    d = _abi.PromptDesc()
    t = np.ascontiguousarray([] if text_ids is None else text_ids, dtype=np.uint32)
    keep.append(t)
    d.text_ids, d.n_text = _ptr(t, u32p), len(t)
    if instruct_ids is not None:
        ins = np.ascontiguousarray(instruct_ids, dtype=np.uint32)
        keep.append(ins)
        d.instruct_ids, d.n_instruct = _ptr(ins, u32p), len(ins)
    d.lang_id, d.spk_id = (-1 if lang_id is None else lang_id), spk_id
    if spk_emb is not None:
        s = np.ascontiguousarray(spk_emb, dtype=np.float32)
        keep.append(s)
        d.spk_emb = _ptr(s, f32p)
    if ref_codes is not None:
        rc = np.ascontiguousarray(ref_codes, dtype=np.int32)
        keep.append(rc)
        d.ref_codes, d.n_ref_frames = _ptr(rc, i32p), rc.size // 16
        rt = np.ascontiguousarray(ref_text_ids if ref_text_ids is not None else [], dtype=np.uint32)
        keep.append(rt)
        d.ref_text_ids, d.n_ref_text = _ptr(rt, u32p), len(rt)
    return d, keep


class GenResult:
    def __init__(self, status, codes, pcm, hit_eos, first_chunk_ms, total_ms, sample_rate):
        self.status, self.codes, self.pcm, self.hit_eos = status, codes, pcm, hit_eos
        self.first_chunk_ms, self.total_ms, self.sample_rate = first_chunk_ms, total_ms, sample_rate
        self._n_frames = None

    @property
    def n_frames(self):
        """The frames the result counts: its codes' rows, or the sum a document's DONE event reports without codes."""
        return self.codes.shape[0] if self._n_frames is None else self._n_frames


class NativeEngine:
    """q3tts_engine handle. One engine per GPU; not re-entrant (same contract as `&mut self`)."""

    def __init__(self, cfg):
        self.lib = _abi.load_library()
        self.cfg = cfg
        self.h = C.c_void_p()
        self._prefixes = weakref.WeakSet()  # destroyed before the engine
        rc = self.lib.q3tts_engine_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_engine_create failed ({rc}): {self.lib.q3tts_last_error(None).decode()}")

    def close(self):
        if getattr(self, "h", None):
            for x in list(getattr(self, "_prefixes", ())):
                x.close()
            self.lib.q3tts_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise _abi.Q3Error(f"{what} failed ({rc}): {self.lib.q3tts_last_error(self.h).decode()}")

    def set_sampler(self, temperature, top_k, top_p, seed=None):
        self._check(self.lib.q3tts_set_sampler(self.h, temperature, top_k, top_p, 0 if seed is None else 1, seed or 0),
                    "q3tts_set_sampler")

    def set_max_steps(self, n):
        self._check(self.lib.q3tts_set_max_steps(self.h, n), "q3tts_set_max_steps")

    def set_predictor_sampler(self, temperature, top_k, top_p):
        """The sampler of codes 1 .. n_codebooks - 1 (q3tts_set_predictor_sampler) for requests admitted from now on; temperature 0 = greedy,
        the default. The reference has no such control (its Predictor is greedy)."""
        self._check(self.lib.q3tts_set_predictor_sampler(self.h, temperature, top_k, top_p), "q3tts_set_predictor_sampler")

    def predictor_sampler(self):
        t, k, p = C.c_float(), C.c_int32(), C.c_float()
        self._check(self.lib.q3tts_get_predictor_sampler(self.h, C.byref(t), C.byref(k), C.byref(p)), "q3tts_get_predictor_sampler")
        return t.value, k.value, p.value

    def set_repetition_penalty(self, p):
        """Repetition penalty on the Talker's code-0 logits over the codes generated so far (q3tts_set_repetition_penalty); 1.0 = off."""
        self._check(self.lib.q3tts_set_repetition_penalty(self.h, p), "q3tts_set_repetition_penalty")

    def repetition_penalty(self):
        p = C.c_float()
        self._check(self.lib.q3tts_get_repetition_penalty(self.h, C.byref(p)), "q3tts_get_repetition_penalty")
        return p.value

    def k_pred_variant(self, force):
        """Test hook: force = 1 runs the sampling form of the frame step whatever the Predictor sampler's temperature."""
        self._check(self.lib.q3tts_k_pred_variant(self.h, int(force)), "q3tts_k_pred_variant")

    def pred_table_row(self, q, code):
        """Test hook (q3tts_k_pred_table_row): row `code` of slice q of the Predictor's layer-0 QKV table (a code out of range: the
        fallback row). Raises Q3Error when the engine has no table."""
        m = self.cfg.model
        out = np.zeros((m.p_n_head + 2 * m.p_n_kv_head) * m.p_head_dim, dtype=np.float32)
        self._check(self.lib.q3tts_k_pred_table_row(self.h, int(q), int(code), _ptr(out, f32p)), "q3tts_k_pred_table_row")
        return out

    def build_prompt(self, desc):
        out, n = f32p(), C.c_int32()
        self._check(self.lib.q3tts_build_prompt(self.h, C.byref(desc), C.byref(out), C.byref(n)), "q3tts_build_prompt")
        d = self.cfg.model.d_embed
        arr = np.ctypeslib.as_array(out, shape=(n.value, d)).copy()
        self.lib.q3tts_free(out)
        return arr

    def create_prefix(self, desc=None, embd=None):
        """A voice prefix (q3tts_prefix_create): the Talker's K/V of a voice part, from a voice-only desc (make_prompt_desc(part="voice"))
        or from host rows [n][d_embed]. Requests that pass it as prefix= give the bits of the whole prompt."""
        if (desc is None) == (embd is None):
            raise ValueError("create_prefix: give exactly one of desc or embd")
        h = C.c_void_p()
        if desc is not None:
            self._check(self.lib.q3tts_prefix_create(self.h, C.byref(desc), None, 0, C.byref(h)), "q3tts_prefix_create")
        else:
            e = np.ascontiguousarray(embd, dtype=np.float32)
            self._check(self.lib.q3tts_prefix_create(self.h, None, _ptr(e, f32p), e.shape[0], C.byref(h)), "q3tts_prefix_create")
        x = NativePrefix(self, h)
        self._prefixes.add(x)
        return x

    @staticmethod
    def make_request(embd=None, desc=None, temperature=0.0, top_k=40, top_p=0.9, seed=None, max_steps=0, min_frames=0,
                     force_eos_at=-1, want_pcm=0, use_engine_sampler=0, prefix=None, text_stream=False, text_open=False):
        """text_stream: the streamed text layout (include/q3tts.h, "streaming text input"; needs desc with at least one text id);
        text_open (sessions only): more text follows through NativeSession.append_text."""
        r = _abi.Request()
        keep = []
        if prefix is not None:
            if not prefix.h:
                raise _abi.Q3Error("the prefix is closed")
            keep.append(prefix)
            r.prefix = prefix.h
        if embd is not None:
            e = np.ascontiguousarray(embd, dtype=np.float32)
            keep.append(e)
            r.prompt_embd, r.n_tok = _ptr(e, f32p), e.shape[0]
        if desc is not None:
            keep.append(desc)
            r.prompt = C.pointer(desc)
        r.use_engine_sampler = use_engine_sampler
        r.temperature, r.top_k, r.top_p = temperature, top_k, top_p
        r.has_seed, r.seed = (0, 0) if seed is None else (1, seed)
        r.max_steps, r.min_frames, r.force_eos_at, r.want_pcm = max_steps, min_frames, force_eos_at, want_pcm
        r.text_stream, r.text_open = int(bool(text_stream)), int(bool(text_open))
        return r, keep

    def _unpack(self, res):
        ncb = self.cfg.model.n_codebooks
        codes = np.ctypeslib.as_array(res.codes, shape=(res.n_frames, ncb)).copy() if res.n_frames > 0 and res.codes else \
            np.zeros((0, ncb), dtype=np.int32)   # (a document's DONE event counts its frames and carries no codes)
        pcm = None
        if res.pcm:
            pcm = np.ctypeslib.as_array(res.pcm, shape=(res.n_samples,)).copy() if res.n_samples > 0 else \
                np.zeros(0, dtype=np.float32)
        out = GenResult(res.status, codes, pcm, bool(res.hit_eos), res.first_chunk_ms, res.total_ms, res.sample_rate)
        out.n_samples = int(res.n_samples)
        if res.n_frames > 0 and not res.codes:
            out._n_frames = int(res.n_frames)
        self.lib.q3tts_result_free(C.byref(res))
        return out

    def generate(self, **kw):
        r, keep = self.make_request(**kw)
        res = _abi.Result()
        self._check(self.lib.q3tts_generate(self.h, C.byref(r), C.byref(res)), "q3tts_generate")
        return self._unpack(res)

    def generate_batch(self, requests):
        """requests: list of kwargs dicts for make_request."""
        n = len(requests)
        arr = (_abi.Request * n)()
        keep = []
        for i, kw in enumerate(requests):
            r, k = self.make_request(**kw)
            arr[i] = r
            keep.append(k)
        res = (_abi.Result * n)()
        self._check(self.lib.q3tts_generate_batch(self.h, arr, n, res), "q3tts_generate_batch")
        return [self._unpack(res[i]) for i in range(n)]

    def set_device_pcm(self, enable=True):
        """Keep every batch's PCM on the device as well (row i of one buffer per generate_batch call): the multi-GPU gather reads it there."""
        self._check(self.lib.q3tts_set_device_pcm(self.h, 1 if enable else 0), "q3tts_set_device_pcm")

    def device_pcm(self):
        """(device pointer, stride in samples, rows) of the last batch's packed PCM; wrap with torch via __cuda_array_interface__."""
        base, stride, n = f32p(), C.c_int64(0), C.c_int32(0)
        self._check(self.lib.q3tts_get_device_pcm(self.h, C.byref(base), C.byref(stride), C.byref(n)), "q3tts_get_device_pcm")
        return (C.cast(base, C.c_void_p).value or 0), int(stride.value), int(n.value)

    def set_output_rate(self, rate):
        """q3tts_set_output_rate: PCM of generate / generate_batch (want_pcm = 1), of streams and of session chunks leaves the engine at
        `rate` Hz, resampled on the device; 0 or the vocoder's own rate = off, the default. Refused while a session or a
        stream is open and while device PCM is enabled. The reference has no such control."""
        self._check(self.lib.q3tts_set_output_rate(self.h, int(rate)), "q3tts_set_output_rate")

    def get_output_rate(self):
        r = C.c_int32(0)
        self._check(self.lib.q3tts_get_output_rate(self.h, C.byref(r)), "q3tts_get_output_rate")
        return r.value

    def resample(self, audio, rate_in, rate_out):
        """q3tts_resample: the finished f32 clip `audio` at rate_in -> ceil(n L / M) samples at rate_out, by the engine's device resampler."""
        a = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        g = math.gcd(int(rate_in), int(rate_out))
        cap = -(-a.size * (int(rate_out) // g) // (int(rate_in) // g)) if g else 0
        out = np.zeros(max(cap, 1), dtype=np.float32)
        n = C.c_int64(0)
        self._check(self.lib.q3tts_resample(self.h, _ptr(a, f32p), a.size, int(rate_in), int(rate_out), _ptr(out, f32p), cap, C.byref(n)), "q3tts_resample")
        return out[:n.value]

    def set_speed(self, permille):
        """q3tts_set_speed: PCM of generate / generate_batch (want_pcm = 1), of streams and of session chunks is time-stretched on the
        device, pitch kept; `permille` in 500..2000 (2000: twice as fast), 0 or 1000 = off, the default. Refused while a
        session or a stream is open and while device PCM is enabled. The reference has no such control."""
        self._check(self.lib.q3tts_set_speed(self.h, int(permille)), "q3tts_set_speed")

    def get_speed(self):
        r = C.c_int32(0)
        self._check(self.lib.q3tts_get_speed(self.h, C.byref(r)), "q3tts_get_speed")
        return r.value

    def time_stretch(self, audio, permille):
        """q3tts_time_stretch: the finished f32 clip `audio` -> ceil(n 1000 / permille) samples, by the engine's device time-stretch."""
        a = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        cap = -(-a.size * 1000 // int(permille)) if int(permille) > 0 else 0
        out = np.zeros(max(cap, 1), dtype=np.float32)
        n = C.c_int64(0)
        self._check(self.lib.q3tts_time_stretch(self.h, _ptr(a, f32p), a.size, int(permille), _ptr(out, f32p), cap, C.byref(n)), "q3tts_time_stretch")
        return out[:n.value]

    def pcm_join(self, clips, kinds, **opts):
        """q3tts_pcm_join: finished host clips and their break kinds (_abi.BREAK_*) -> (the joined f32 PCM, edges [n][4] = lo, hi, begin,
        end), trimmed, faded and laid out by the two device kernels of DESIGN.md §26; opts: the fields of q3tts_join_opts."""
        arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
        n = len(arrs)
        ptrs = (f32p * max(n, 1))(*[_ptr(a, f32p) for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.int64)
        kd = np.ascontiguousarray(kinds, dtype=np.int32)
        if kd.shape != (n,):
            raise ValueError("pcm_join: kinds takes one value per clip")
        o = join_opts(**opts)
        cap = int(lens.sum()) + max(n - 1, 0) * max(o.pause_ms) * (self.cfg.vocoder.sample_rate // 1000 + 1)
        out = np.zeros(max(cap, 1), dtype=np.float32)
        edges = np.zeros((max(n, 1), 4), dtype=np.int64)
        n_out = C.c_int64(0)
        i64p = C.POINTER(C.c_int64)
        self._check(self.lib.q3tts_pcm_join(self.h, ptrs, _ptr(lens, i64p), _ptr(kd, i32p), n, C.byref(o), _ptr(out, f32p), cap, C.byref(n_out),
                                            _ptr(edges, i64p)), "q3tts_pcm_join")
        return out[:n_out.value], edges[:n]

    def generate_long(self, segments, voice=None, prefix=None, speed_permille=0, output_rate=0, join=None, **template_kw):
        """q3tts_generate_long: `segments` is a list of (ids, kind) or (ids, kind, max_steps); exactly one of voice (a voice-only desc) and
        prefix (a NativePrefix); template_kw are make_request's sampler fields, min_frames, force_eos_at and max_steps; join: a dict of
        q3tts_join_opts fields. Returns a GenResult-like object: pcm, n_samples, sample_rate, n_truncated, generate_ms / join_ms / total_ms
        and info, one dict per segment (status, n_frames, hit_eos, n_native, lo, hi, begin, end, out_begin, out_end). A segment that fails
        by itself raises Q3Error; the error's `info` attribute then holds the per-segment statuses."""
        tmpl, keep = self.make_request(**template_kw)
        n = len(segments)
        segs = (_abi.LongSegment * max(n, 1))()
        for i, sg in enumerate(segments):
            ids = np.ascontiguousarray(sg[0], dtype=np.uint32)
            keep.append(ids)
            segs[i].ids, segs[i].n_ids, segs[i].kind = _ptr(ids, u32p), ids.size, int(sg[1])
            segs[i].max_steps = int(sg[2]) if len(sg) > 2 else 0
        o = _abi.LongOpts()
        o.join = join_opts(**(join or {}))
        o.speed_permille, o.output_rate = int(speed_permille), int(output_rate)
        if prefix is not None and not prefix.h:
            raise _abi.Q3Error("the prefix is closed")
        res = _abi.LongResult()
        rc = self.lib.q3tts_generate_long(self.h, C.byref(tmpl), C.byref(voice) if voice is not None else None,
                                          prefix.h if prefix is not None else None, segs, n, C.byref(o), C.byref(res))
        names = [f[0] for f in _abi.LongInfo._fields_]
        info = [{k: int(getattr(res.info[i], k)) for k in names} for i in range(res.n_segments)] if res.info else []
        try:
            if rc != 0:
                err = _abi.Q3Error(f"q3tts_generate_long failed ({rc}): {self.lib.q3tts_last_error(self.h).decode()}")
                err.status, err.info, err.pcm_is_null = rc, info, not bool(res.pcm)
                raise err
            pcm = np.ctypeslib.as_array(res.pcm, shape=(res.n_samples,)).copy() if res.n_samples > 0 else np.zeros(0, dtype=np.float32)
            out = GenResult(res.status, np.zeros((0, self.cfg.model.n_codebooks), dtype=np.int32), pcm, res.n_truncated == 0, 0.0, res.total_ms, res.sample_rate)
            out.n_samples, out.n_truncated, out.info = int(res.n_samples), int(res.n_truncated), info
            out.generate_ms, out.join_ms = float(res.generate_ms), float(res.join_ms)
            return out
        finally:
            self.lib.q3tts_long_result_free(C.byref(res))

    def vocoder_bench(self, n_slots, chunks):
        ms = C.c_float(0)
        self._check(self.lib.q3tts_k_vocoder_bench(self.h, n_slots, chunks, C.byref(ms)), "q3tts_k_vocoder_bench")
        return ms.value

    def row_buckets(self):
        """The engine's row buckets (q3tts_k_row_buckets of its max_batch)."""
        return row_buckets(self.cfg.max_batch)

    def bucket_steps(self):
        """{bucket rows: frame steps run on it since the engine was created} (q3tts_k_bucket_steps)."""
        out = (C.c_int64 * 32)()
        n = self.lib.q3tts_k_bucket_steps(self.h, out, 32)
        if n < 0:
            raise _abi.Q3Error("q3tts_k_bucket_steps failed")
        return dict(zip(self.row_buckets(), [int(out[i]) for i in range(n)]))

    def prefix_stats(self):
        """(k_kv_prefix launches since creation, the most prefixed requests one prefill group has held) — q3tts_k_prefix_stats."""
        o = (C.c_int64 * 2)()
        self._check(self.lib.q3tts_k_prefix_stats(self.h, o), "q3tts_k_prefix_stats")
        return int(o[0]), int(o[1])

    @property
    def vocoder_source(self):
        """q3tts_get_vocoder_source: 0 = no vocoder, 1 = seeded synthetic weights, 2 = the file qwen3_tts_vocoder.gguf."""
        s = C.c_int32(0)
        self._check(self.lib.q3tts_get_vocoder_source(self.h, C.byref(s)), "q3tts_get_vocoder_source")
        return int(s.value)

    def device_bytes(self):
        """Device bytes the engine's allocator has handed out (q3tts_k_device_bytes)."""
        b = C.c_int64(0)
        self._check(self.lib.q3tts_k_device_bytes(self.h, C.byref(b)), "q3tts_k_device_bytes")
        return int(b.value)

    def timings(self):
        t = _abi.Timings()
        self._check(self.lib.q3tts_get_timings(self.h, C.byref(t)), "q3tts_get_timings")
        return t

    def mel(self, audio):
        """24 kHz mono f32 -> [n_frames][128] log-mel (the clone path's front-end)."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        cap = int(self.lib.q3tts_mel_frames(a.size))
        out = np.zeros((max(cap, 1), 128), dtype=np.float32)
        n = C.c_int32(0)
        self._check(self.lib.q3tts_mel(self.h, _ptr(a, f32p) if a.size else None, a.size, _ptr(out, f32p), cap, C.byref(n)), "q3tts_mel")
        return out[:n.value].copy()

    # voice-clone encoders (q3_clone.hip) ----------------------------------------------------------
    def clone_init(self, ccfg):
        self._check(self.lib.q3tts_clone_init(self.h, C.byref(ccfg)), "q3tts_clone_init")
        self.clone_cfg = ccfg

    def clone_load(self, dir=None):
        """q3tts_clone_load: both encoders from qwen3_tts_speaker_encoder.gguf and qwen3_tts_codec_encoder.gguf, found in `dir` or its
        parent (None: the engine's own weights_path). clone_cfg becomes the shape the files state."""
        wdir = None if dir is None else os.fsencode(dir)
        self._check(self.lib.q3tts_clone_load(self.h, wdir), "q3tts_clone_load")
        if wdir is None:
            wdir = self.cfg.weights_path
        self.clone_cfg = clone_config_from_dir(wdir)

    @property
    def clone_source(self):
        """q3tts_get_clone_source: 0 = encoders not loaded, 1 = seeded synthetic weights (clone_init), 2 = the two files (clone_load)."""
        s = C.c_int32(0)
        self._check(self.lib.q3tts_get_clone_source(self.h, C.byref(s)), "q3tts_get_clone_source")
        return int(s.value)

    def clone_audio_frames(self, n_samples):
        return int(self.lib.q3tts_clone_audio_frames(self.h, int(n_samples)))

    def _clone_codebooks(self):
        c = getattr(self, "clone_cfg", None)
        return c.ae_n_codebooks if c is not None else 16

    def audio_encode(self, audio):
        """AudioEncoder::encode: 24 kHz mono f32 -> i64 codes [n_frames][n_codebooks]."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        cap = max(self.clone_audio_frames(a.size), 1)
        ncb = self._clone_codebooks()
        out = np.zeros((cap, ncb), dtype=np.int64)
        n = C.c_int32(0)
        self._check(self.lib.q3tts_clone_audio_encode(self.h, _ptr(a, f32p) if a.size else None, a.size,
                                                      out.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n)), "q3tts_clone_audio_encode")
        return out[:n.value].copy()

    def audio_latent(self, audio):
        a = np.ascontiguousarray(audio, dtype=np.float32)
        cap = max(self.clone_audio_frames(a.size), 1)
        out = np.zeros((cap, self.clone_cfg.ae_hidden), dtype=np.float32)
        n = C.c_int32(0)
        self._check(self.lib.q3tts_k_audio_latent(self.h, _ptr(a, f32p) if a.size else None, a.size, _ptr(out, f32p), cap, C.byref(n)),
                    "q3tts_k_audio_latent")
        return out[:n.value].copy()

    def speaker_encode(self, audio):
        """SpeakerEncoder::encode: 24 kHz mono f32 -> [se_dim] (log-mel on the device, then the encoder)."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        c = getattr(self, "clone_cfg", None)
        out = np.zeros(c.se_dim if c is not None else self.cfg.model.d_embed, dtype=np.float32)
        self._check(self.lib.q3tts_clone_speaker_encode(self.h, _ptr(a, f32p) if a.size else None, a.size, _ptr(out, f32p)),
                    "q3tts_clone_speaker_encode")
        return out

    def speaker_from_mel(self, mel):
        m = np.ascontiguousarray(mel, dtype=np.float32)
        out = np.zeros(self.clone_cfg.se_dim, dtype=np.float32)
        self._check(self.lib.q3tts_k_speaker_from_mel(self.h, _ptr(m, f32p), m.shape[0], _ptr(out, f32p)), "q3tts_k_speaker_from_mel")
        return out

    def probe(self, enable):
        """Measurement mode (bench.py): eager frame steps with HIP events around one GEMM per frame — 2 (or True): the Talker's
        layer-0 gate/up (exact kernel); 1: the Predictor's pass-1 gate/up (bf16-MFMA kernel); 0 / False: off."""
        mode = 2 if enable is True else int(enable)
        self._check(self.lib.q3tts_k_probe(self.h, mode), "q3tts_k_probe")

    def alloc_upload_mismatches(self, nbytes):
        """Allocator contract hook (q3tts_k_alloc_upload): bytes that read back wrong after a null-stream upload right behind the allocation."""
        bad = C.c_int64(-1)
        self._check(self.lib.q3tts_k_alloc_upload(self.h, int(nbytes), C.byref(bad)), "q3tts_k_alloc_upload")
        return int(bad.value)

    def talker_prefill(self, embd):
        e = np.ascontiguousarray(embd, dtype=np.float32)
        hid = np.zeros(self.cfg.model.t_d_model, dtype=np.float32)
        lg = np.zeros(self.cfg.model.t_vocab, dtype=np.float32)
        self._check(self.lib.q3tts_k_talker_prefill(self.h, _ptr(e, f32p), e.shape[0], _ptr(hid, f32p), _ptr(lg, f32p)),
                    "q3tts_k_talker_prefill")
        return hid, lg

    def talker_prefill_prefix(self, prefix, embd):
        """talker_prefill over prefix rows ++ embd (q3tts_k_talker_prefill_prefix)."""
        e = np.ascontiguousarray(embd, dtype=np.float32)
        hid = np.zeros(self.cfg.model.t_d_model, dtype=np.float32)
        lg = np.zeros(self.cfg.model.t_vocab, dtype=np.float32)
        self._check(self.lib.q3tts_k_talker_prefill_prefix(self.h, prefix.h, _ptr(e, f32p), e.shape[0], _ptr(hid, f32p), _ptr(lg, f32p)),
                    "q3tts_k_talker_prefill_prefix")
        return hid, lg

    def vocoder(self, codes, chunk_frames=0):
        c = np.ascontiguousarray(codes, dtype=np.int32)
        spf = 1
        v = self.cfg.vocoder
        for i in range(v.n_upsample):
            spf *= v.upsample_ratios[i]
        for i in range(v.n_dec_blocks):
            spf *= v.dec_rates[i]
        pcm = np.zeros(c.shape[0] * spf + 16, dtype=np.float32)
        ns = C.c_int32()
        self._check(self.lib.q3tts_k_vocoder(self.h, _ptr(c, i32p), c.shape[0], chunk_frames, _ptr(pcm, f32p), C.byref(ns)),
                    "q3tts_k_vocoder")
        return pcm[:ns.value].copy()

    def vocoder_latent(self, codes, chunk_frames=0):
        """The vocoder transformer's f32 residual rows after its last layer (before the final norm), [n_frames][latent_dim]: slot 0
        driven as vocoder() drives it (q3tts_k_vocoder_latent)."""
        c = np.ascontiguousarray(codes, dtype=np.int32)
        out = np.zeros((c.shape[0], self.cfg.vocoder.latent_dim), dtype=np.float32)
        self._check(self.lib.q3tts_k_vocoder_latent(self.h, _ptr(c, i32p), c.shape[0], chunk_frames, _ptr(out, f32p)), "q3tts_k_vocoder_latent")
        return out

    def vocoder_taps(self, codes, chunk_frames=0, tap_call=0, buf_bytes=160 << 20):
        """Every tap of vocoder call `tap_call` (slot 0 driven as vocoder() drives it; calls of <= 4 frames numbered from 0; the drive ends
        after that call): the front half (embedding sum, pre-conv, each transformer layer's stages and slot 0's whole K / V ring, the final
        norm) and the convolution half, as {name: (array[hist_rows + rows][channels], hist_rows)}: f32 taps as float32, bf16 taps as uint16
        bits, A-tiled taps untiled (q3tts_k_vocoder_taps; the names are listed in include/q3tts.h). More than 256 taps or buf_bytes is an
        error, never a cut."""
        c = np.ascontiguousarray(codes, dtype=np.int32)
        buf = np.empty(buf_bytes, dtype=np.uint8)
        recs = (_abi.VocTap * 256)()
        n = C.c_int32()
        self._check(self.lib.q3tts_k_vocoder_taps(self.h, _ptr(c, i32p), c.shape[0], chunk_frames, tap_call, buf.ctypes.data, buf.size, recs, 256,
                                                  C.byref(n)), "q3tts_k_vocoder_taps")
        out = {}
        for r in recs[:n.value]:
            H, T, K = r.hist_rows, r.rows, r.channels
            dt = np.uint16 if r.dtype else np.float32
            if r.layout:   # q3_atile_off(row, k, K / 32), csrc/q3_kernels.h
                flat = np.frombuffer(buf, dtype=dt, count=((H + T + 15) // 16) * 16 * K, offset=r.offset)
                row, k = np.arange(H + T)[:, None], np.arange(K)[None, :]
                cc = k & 31
                off = ((((row >> 4) * (K >> 5) + (k >> 5)) * 64 + ((cc & 15) >> 2) * 16 + (row & 15)) << 3) + (cc & 3) + ((cc & 16) >> 2)
                a = flat[off]
            else:
                a = np.frombuffer(buf, dtype=dt, count=(H + T) * K, offset=r.offset).reshape(H + T, K).copy()
            out[r.name.decode()] = (a, H)
        return out


class NativePrefix:
    """q3tts_prefix: a voice part's Talker K/V on the device of one engine (NativeEngine.create_prefix). close() is refused while a session
    is open on the engine; the engine closes its prefixes when it closes."""

    def __init__(self, engine: NativeEngine, h, session=None):
        self.engine, self.lib, self.h = engine, engine.lib, h
        self.session = session   # the NativeSession that made it (create_prefix / submit(keep_voice=True)): pending until its PREFIX event
        self._n_rows = int(self.lib.q3tts_prefix_rows(h))

    @property
    def n_rows(self):
        """The prefix's rows; 0 while a session's prefix is pending (or when it failed)."""
        if not self._n_rows and getattr(self, "h", None):
            self._n_rows = int(self.lib.q3tts_prefix_rows(self.h))
        return self._n_rows

    @property
    def state(self):
        """q3tts_prefix_state: 0 pending, 1 ready, < 0 the status it failed with."""
        if not getattr(self, "h", None):
            raise _abi.Q3Error("the prefix is closed")
        return int(self.lib.q3tts_prefix_state(self.h))

    def close(self):
        """Gives the handle back, once: released to its session while that is open, destroyed otherwise."""
        if getattr(self, "h", None):
            sess = self.session
            if sess is not None and getattr(sess, "h", None):
                sess._check(self.lib.q3tts_session_prefix_release(sess.h, self.h), "q3tts_session_prefix_release")
            else:
                self.engine._check(self.lib.q3tts_prefix_destroy(self.h), "q3tts_prefix_destroy")
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except _abi.Q3Error:  # a session still open on the engine: the engine frees it when it closes
            pass


class NativeSession:
    """q3tts_session_*: continuous batching with per-request streaming on one engine (include/q3tts.h, "sessions"). The session owns the
    engine until close(); submit() and cancel() may be called from any thread, events() from one consumer thread."""

    def __init__(self, engine: NativeEngine, pcm_format=_abi.PCM_F32, swap_mb=0):
        """swap_mb > 0 (q3tts_session_set_swap): a device arena of that many MiB that parked requests are swapped out into while others
        wait for their slots (include/q3tts.h, "paced requests and swapping"). A fraction is allowed."""
        self.engine, self.lib = engine, engine.lib
        self.dtype = np.int16 if pcm_format == _abi.PCM_I16 else np.float32
        self._ctype = C.c_int16 if pcm_format == _abi.PCM_I16 else C.c_float
        self._open = set()   # ids without their final event yet
        self.h = C.c_void_p()
        engine._check(self.lib.q3tts_session_create(engine.h, pcm_format, C.byref(self.h)), "q3tts_session_create")
        if swap_mb:
            try:
                self.set_swap(int(swap_mb * (1 << 20)))
            except _abi.Q3Error:
                self.close()
                raise

    def _check(self, rc, what):
        if rc != 0:
            raise _abi.Q3Error(f"{what} failed ({rc}): {self.lib.q3tts_session_last_error(self.h).decode()}")

    @property
    def open_ids(self):
        """The ids submitted through this object whose final event next() has not returned yet."""
        return frozenset(self._open)

    def set_swap(self, arena_bytes):
        """q3tts_session_set_swap: the swap arena's size in bytes (0: off), before the first submission."""
        self._check(self.lib.q3tts_session_set_swap(self.h, int(arena_bytes)), "q3tts_session_set_swap")

    def grant(self, rid, frames):
        """q3tts_session_grant: frames > 0 more frames of credit for a request submitted with credit_frames; frames < 0 lifts its limit.
        Thread-safe."""
        self._check(self.lib.q3tts_session_grant(self.h, rid, int(frames)), "q3tts_session_grant")

    def swap_stats(self):
        """q3tts_session_swap_stats as a dict: swap_outs, swap_ins, moved (swap-ins into another slot), arena_used, arena_peak (bytes),
        skipped (swap-outs the arena had no room for)."""
        out = (C.c_int64 * 6)()
        self._check(self.lib.q3tts_session_swap_stats(self.h, out), "q3tts_session_swap_stats")
        return dict(zip(("swap_outs", "swap_ins", "moved", "arena_used", "arena_peak", "skipped"), (int(v) for v in out)))

    def swap_phase_ms(self):
        """q3tts_k_swap_phase_ms: (host ms in swap_out, host ms in swap_in, boundaries that moved a block) so far."""
        out = (C.c_double * 3)()
        self._check(self.lib.q3tts_k_swap_phase_ms(self.h, out), "q3tts_k_swap_phase_ms")
        return float(out[0]), float(out[1]), int(out[2])

    def submit(self, keep_voice=False, voice_rows=0, credit_frames=None, **request_kw):
        """credit_frames (q3tts_session_submit_paced): the request is paced — it takes its next 4 frames only while n_frames + 4 <= its
        credit, which starts at credit_frames (>= 4) and grows through grant(). Not with keep_voice.
        request_kw: NativeEngine.make_request keywords, prefix=, text_stream= and text_open= included (want_pcm is ignored: a session
        always produces PCM). Returns the id.
        keep_voice=True (q3tts_session_submit_keep_voice): a whole-prompt request whose voice part becomes a prefix without a second
        prefill — voice_rows rows of it, 0 = the voice part of desc. Returns (id, prefix): the prefix is pending until its EV_PREFIX
        event, and requests may name it at once."""
        if not self.h:
            raise _abi.Q3Error("q3tts_session_submit: the session is closed")
        r, keep = NativeEngine.make_request(**request_kw)
        rid = C.c_uint64(0)
        if credit_frames is not None:
            if keep_voice:
                raise ValueError("submit: credit_frames and keep_voice do not combine")
            self._check(self.lib.q3tts_session_submit_paced(self.h, C.byref(r), int(credit_frames), C.byref(rid)), "q3tts_session_submit_paced")
            self._open.add(rid.value)
            return rid.value
        if not keep_voice:
            self._check(self.lib.q3tts_session_submit(self.h, C.byref(r), C.byref(rid)), "q3tts_session_submit")
            self._open.add(rid.value)
            return rid.value
        h = C.c_void_p()
        self._check(self.lib.q3tts_session_submit_keep_voice(self.h, C.byref(r), int(voice_rows), C.byref(rid), C.byref(h)),
                    "q3tts_session_submit_keep_voice")
        self._open.add(rid.value)
        return rid.value, self._adopt(h)

    def _adopt(self, h):
        x = NativePrefix(self.engine, h, session=self)
        self.engine._prefixes.add(x)
        return x

    def create_prefix(self, desc=None, embd=None):
        """q3tts_session_prefix_create: a prefix job in the running batch, arguments as NativeEngine.create_prefix. Returns (id, prefix);
        its one event is EV_PREFIX (is_final) with the job's status."""
        if (desc is None) == (embd is None):
            raise ValueError("create_prefix: give exactly one of desc or embd")
        h, rid = C.c_void_p(), C.c_uint64(0)
        if desc is not None:
            rc = self.lib.q3tts_session_prefix_create(self.h, C.byref(desc), None, 0, C.byref(h), C.byref(rid))
        else:
            e = np.ascontiguousarray(embd, dtype=np.float32)
            rc = self.lib.q3tts_session_prefix_create(self.h, None, _ptr(e, f32p), e.shape[0], C.byref(h), C.byref(rid))
        self._check(rc, "q3tts_session_prefix_create")
        self._open.add(rid.value)
        return rid.value, self._adopt(h)

    def release_prefix(self, x):
        """q3tts_session_prefix_release: gives a prefix back during the session, in any state; the store is freed once no queued request
        names it. Also takes a prefix made before the session opened."""
        if not x.h:
            raise _abi.Q3Error("the prefix is closed")
        self._check(self.lib.q3tts_session_prefix_release(self.h, x.h), "q3tts_session_prefix_release")
        x.h = None

    def clone_voice(self, audio, rate=24000):
        """q3tts_session_clone: (codes i64 [n_frames][n_codebooks], speaker embedding) of a mono f32 clip at `rate` Hz, encoded between two
        chunk boundaries while the batch runs; blocks. The bits of NativeEngine.audio_encode / speaker_encode outside a session."""
        a = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        n24 = a.size if rate == 24000 else -(-a.size * (24000 // math.gcd(int(rate), 24000)) // (int(rate) // math.gcd(int(rate), 24000)))
        cap = max(self.engine.clone_audio_frames(n24), 1)
        codes = np.zeros((cap, self.engine._clone_codebooks()), dtype=np.int64)
        c = getattr(self.engine, "clone_cfg", None)
        spk = np.zeros(c.se_dim if c is not None else self.engine.cfg.model.d_embed, dtype=np.float32)
        n = C.c_int32(0)
        self._check(self.lib.q3tts_session_clone(self.h, _ptr(a, f32p) if a.size else None, a.size, int(rate),
                                                 codes.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n), _ptr(spk, f32p)), "q3tts_session_clone")
        return codes[:n.value].copy(), spk

    @staticmethod
    def _doc_segments(segments, keep):
        n = len(segments)
        segs = (_abi.LongSegment * max(n, 1))()
        for i, sg in enumerate(segments):
            ids = np.ascontiguousarray(sg[0], dtype=np.uint32)
            keep.append(ids)
            segs[i].ids, segs[i].n_ids, segs[i].kind = _ptr(ids, u32p), ids.size, int(sg[1])
            segs[i].max_steps = int(sg[2]) if len(sg) > 2 else 0
        return segs, n

    def submit_document(self, segments, voice=None, prefix=None, join=None, ahead=0, open=False, speed_permille=0, output_rate=0, **template_kw):
        """q3tts_session_submit_document: `segments` as NativeEngine.generate_long takes them ((ids, kind) or (ids, kind, max_steps));
        exactly one of voice (a voice-only desc) and prefix (a NativePrefix, ready or pending); join: a dict of q3tts_join_opts fields;
        ahead: how many segments may run in front of the one being delivered (0: 8); open=True: more segments follow through
        append_document. speed_permille / output_rate: the document's own, as generate_long's (0: off). template_kw: make_request's
        sampler fields, min_frames, force_eos_at, max_steps. Returns the document's id: its EV_CHUNK payloads joined are generate_long's
        pcm for the same options bit for bit; EV_SEGMENT events carry each segment's result (res.segment = its index)."""
        if not self.h:
            raise _abi.Q3Error("q3tts_session_submit_document: the session is closed")
        tmpl, keep = NativeEngine.make_request(**template_kw)
        segs, n = self._doc_segments(segments, keep)
        o = doc_opts(ahead=ahead, open=1 if open else 0, speed_permille=speed_permille, output_rate=output_rate, **(join or {}))
        if prefix is not None and not prefix.h:
            raise _abi.Q3Error("the prefix is closed")
        did = C.c_uint64(0)
        self._check(self.lib.q3tts_session_submit_document(self.h, C.byref(tmpl), C.byref(voice) if voice is not None else None,
                                                           prefix.h if prefix is not None else None, segs, n, C.byref(o), C.byref(did)),
                    "q3tts_session_submit_document")
        self._open.add(did.value)
        return did.value

    def append_document(self, did, segments, close=False):
        """q3tts_session_document_append: more segments for a document submitted with open=True; close=True ends it (segments may be empty)."""
        keep = []
        segs, n = self._doc_segments(segments, keep)
        self._check(self.lib.q3tts_session_document_append(self.h, did, segs, n, 1 if close else 0), "q3tts_session_document_append")

    def document_info(self, did):
        """q3tts_session_document_info: (info, n_delivered) — one dict per segment delivered so far (generate_long's info fields) and the
        samples handed out so far. Thread-safe."""
        cap = 64
        while True:
            arr = (_abi.LongInfo * cap)()
            n, nd = C.c_int32(0), C.c_int64(0)
            self._check(self.lib.q3tts_session_document_info(self.h, did, arr, cap, C.byref(n), C.byref(nd)), "q3tts_session_document_info")
            if n.value <= cap:
                names = [f[0] for f in _abi.LongInfo._fields_]
                return [{k: int(getattr(arr[i], k)) for k in names} for i in range(n.value)], int(nd.value)
            cap = n.value + 64

    def doc_mem_cap(self, nbytes):
        """q3tts_k_session_doc_mem_cap (test hook): documents are accepted as if the device had at most nbytes free; < 0: off."""
        self._check(self.lib.q3tts_k_session_doc_mem_cap(self.h, int(nbytes)), "q3tts_k_session_doc_mem_cap")

    def cancel(self, rid):
        self._check(self.lib.q3tts_session_cancel(self.h, rid), "q3tts_session_cancel")

    def append_text(self, rid, ids, close=False):
        """q3tts_session_append_text: more text ids for a request submitted with text_stream=True, text_open=True; close=True ends its text
        (ids may then be empty). Thread-safe."""
        t = np.ascontiguousarray([] if ids is None else ids, dtype=np.uint32)
        self._check(self.lib.q3tts_session_append_text(self.h, rid, _ptr(t, u32p) if t.size else None, t.size, 1 if close else 0),
                    "q3tts_session_append_text")

    def next(self, timeout_ms=-1):
        """One event as (id, kind, pcm ndarray | None, is_final, GenResult | None), or None on timeout. EV_SEGMENT (documents): the result is
        the segment's own, res.segment its index, res.n_samples its piece's length. EV_PREFIX (only after create_prefix
        or submit(keep_voice=True)): the result's status is the prefix's; it is final for a job, not for a keep-voice request."""
        ev = _abi.SessionEvent()
        self._check(self.lib.q3tts_session_next(self.h, timeout_ms, C.byref(ev)), "q3tts_session_next")
        if ev.kind == _abi.EV_NONE:
            return None
        pcm = res = None
        if ev.kind == _abi.EV_CHUNK:
            pcm = np.ctypeslib.as_array(C.cast(ev.pcm, C.POINTER(self._ctype)), shape=(ev.n_samples,)).copy() if ev.n_samples > 0 else \
                np.zeros(0, dtype=self.dtype)
        else:
            res = self.engine._unpack(ev.result)
            if ev.kind == _abi.EV_SEGMENT:
                res.segment = int(ev.n_samples)
            if ev.is_final:
                self._open.discard(ev.id)
        return ev.id, ev.kind, pcm, bool(ev.is_final), res

    def events(self, timeout_ms=-1):
        """Generator over next(): ends when every submitted id has had its final event, or when timeout_ms passes without one."""
        while self._open:
            ev = self.next(timeout_ms)
            if ev is None:
                return
            yield ev

    def close(self):
        if getattr(self, "h", None):
            self.lib.q3tts_session_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


# ---- kernel-level hooks (host arrays in / out) -------------------------------------------------

def engine_footprint(cfg):
    """q3tts_k_engine_footprint: the device bytes q3tts_engine_create checks against the free memory for cfg (needs no GPU)."""
    b = C.c_int64(0)
    rc = _abi.load_library().q3tts_k_engine_footprint(C.byref(cfg), C.byref(b))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_engine_footprint failed ({rc}): {_abi.load_library().q3tts_last_error(None).decode()}")
    return int(b.value)


def row_buckets(max_batch):
    """q3tts_k_row_buckets: the row buckets of an engine with max_batch slots (needs no GPU). Raises Q3Error outside 1..256."""
    out = (C.c_int32 * 32)()
    n = _abi.load_library().q3tts_k_row_buckets(max_batch, out, 32)
    if n < 0:
        raise _abi.Q3Error(f"q3tts_k_row_buckets({max_batch}) failed ({n})")
    return [int(out[i]) for i in range(n)]


class NativeNode:
    """q3tts_node_*: one engine + one host thread per listed GPU inside the library, requests sharded by index (i mod G), the PCM of a
    batch optionally gathered to the first device as i16 over RCCL (include/q3tts.h)."""

    def __init__(self, cfg, devices):
        self.lib = _abi.load_library()
        self.cfg = cfg
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        self.h = C.c_void_p()
        rc = self.lib.q3tts_node_create(C.byref(cfg), arr, len(self.devices), C.byref(self.h))
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_node_create failed ({rc}): {self.lib.q3tts_node_last_error(None).decode()}")

    def close(self):
        if self.h:
            self.lib.q3tts_node_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        self.close()

    def generate_batch(self, requests, gather_i16=False):
        """requests: kwargs dicts for NativeEngine.make_request. Returns GenResult list; with gather_i16 every result carries .pcm_i16
        (np.int16, gathered through device 0) instead of .pcm."""
        n = len(requests)
        arr = (_abi.Request * n)()
        keep = []
        for i, kw in enumerate(requests):
            r, k = NativeEngine.make_request(**kw)
            arr[i] = r
            keep.append(k)
        res = (_abi.Result * n)()
        i16 = (C.POINTER(C.c_int16) * n)() if gather_i16 else None
        rc = self.lib.q3tts_node_generate_batch(self.h, arr, n, res, i16)
        if rc != 0:
            self.last_failed_statuses = [int(res[i].status) for i in range(n)]
            for i in range(n):   # (the contract: every result is valid to free, whatever the return code; no i16 buffer is left allocated)
                self.lib.q3tts_result_free(C.byref(res[i]))
            assert not gather_i16 or not any(bool(i16[i]) for i in range(n))
            raise _abi.Q3Error(f"q3tts_node_generate_batch failed ({rc}): {self.lib.q3tts_node_last_error(self.h).decode()}")
        ncb = self.cfg.model.n_codebooks
        outs = []
        for i in range(n):
            r = res[i]
            codes = np.ctypeslib.as_array(r.codes, shape=(r.n_frames, ncb)).copy() if r.n_frames > 0 else np.zeros((0, ncb), dtype=np.int32)
            pcm = np.ctypeslib.as_array(r.pcm, shape=(r.n_samples,)).copy() if (r.pcm and r.n_samples > 0) else None
            o = GenResult(r.status, codes, pcm, bool(r.hit_eos), r.first_chunk_ms, r.total_ms, r.sample_rate)
            o.n_samples = int(r.n_samples)
            o.pcm_i16 = None
            if gather_i16 and i16[i]:
                o.pcm_i16 = np.ctypeslib.as_array(i16[i], shape=(r.n_samples,)).copy()
                self.lib.q3tts_free(C.cast(i16[i], C.c_void_p))
            self.lib.q3tts_result_free(C.byref(r))
            outs.append(o)
        return outs

    def timings(self):
        t = _abi.NodeTimings()
        self.lib.q3tts_node_get_timings(self.h, C.byref(t))
        return t


def node_shard(n_total, world, rank):
    """q3tts_node_shard (host only): the global request indices device `rank` of `world` owns, in order."""
    lib = _abi.load_library()
    k = lib.q3tts_node_shard(n_total, world, rank, None, 0)
    if k < 0:
        raise ValueError("bad shard arguments")
    idx = np.zeros(max(k, 1), dtype=np.int32)
    lib.q3tts_node_shard(n_total, world, rank, _ptr(idx, i32p), k)
    return idx[:k].tolist()


def k_gemm_exact(x, w_bf16, norm_w=None, eps=1e-6, bias=None, epilogue=0, y_in=None, device=0, iters=0):
    lib = _abi.load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w_bf16, dtype=np.uint16)
    B, K = x.shape
    N = w.shape[0]
    ny = N // 2 if epilogue == 2 else N
    y = np.zeros((B, ny), dtype=np.float32) if y_in is None else np.ascontiguousarray(y_in, dtype=np.float32).copy()
    keys = np.zeros(B, dtype=np.uint64)
    ms = C.c_float(0)
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, dtype=np.float32)
    bs = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    rc = lib.q3tts_k_gemm_exact(device, _ptr(x, f32p), B, K, w.ctypes.data_as(C.POINTER(C.c_uint16)), N,
                                None if nw is None else _ptr(nw, f32p), eps, None if bs is None else _ptr(bs, f32p),
                                epilogue, _ptr(y, f32p), keys.ctypes.data_as(C.POINTER(C.c_uint64)), iters, C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_gemm_exact failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return y, keys, ms.value


def k_bgemm(xb, wb, ssp, d_norm, eps, epi, nw_next=None, y0=None, device=0, iters=0):
    """The decoder's GEMM through its launcher (q3tts_k_bgemm): natural-order bf16 bit arrays in, the epilogue's outputs out."""
    lib = _abi.load_library()
    xb = np.ascontiguousarray(xb, dtype=np.uint16); wb = np.ascontiguousarray(wb, dtype=np.uint16)
    B, K = xb.shape
    N = wb.shape[0]
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yb = np.zeros((B, N // 2 if epi == 2 else N), dtype=np.uint16)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    keys = np.zeros(B, dtype=np.uint64)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    ms = C.c_float(0)
    rc = lib.q3tts_k_bgemm(device, xb.ctypes.data, B, K, wb.ctypes.data, N, None if sp is None else sp.ctypes.data, 0 if sp is None else sp.shape[1],
                           d_norm, eps, epi, None if nw is None else nw.ctypes.data, y.ctypes.data, yb.ctypes.data, sso.ctypes.data, keys.ctypes.data,
                           iters, C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_bgemm failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return dict(y=y, yb=yb, ssp_out=sso, keys=keys, ms=ms.value)


def k_bgemm_q8(xb, q, d16, ssp, d_norm, eps, epi, nw_next=None, y0=None, device=0, iters=0):
    """The same launch with ggml Q8_0 weights kept in block form on the device (q3tts_k_bgemm_q8): q int8 [N][K], d16 f16 bits [N][K/32]."""
    lib = _abi.load_library()
    xb = np.ascontiguousarray(xb, dtype=np.uint16); q = np.ascontiguousarray(q, dtype=np.int8); d16 = np.ascontiguousarray(d16, dtype=np.uint16)
    B, K = xb.shape
    N = q.shape[0]
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yb = np.zeros((B, N // 2 if epi == 2 else N), dtype=np.uint16)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    keys = np.zeros(B, dtype=np.uint64)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    ms = C.c_float(0)
    rc = lib.q3tts_k_bgemm_q8(device, xb.ctypes.data, B, K, q.ctypes.data, d16.ctypes.data, N, None if sp is None else sp.ctypes.data,
                              0 if sp is None else sp.shape[1], d_norm, eps, epi, None if nw is None else nw.ctypes.data, y.ctypes.data, yb.ctypes.data,
                              sso.ctypes.data, keys.ctypes.data, iters, C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_bgemm_q8 failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return dict(y=y, yb=yb, ssp_out=sso, keys=keys, ms=ms.value)


def k_bgemm_q8a8_argmax(aq, ad, q, d16, ssp, d_norm, eps, device=0):
    """The W8A8 GEMM with the ARGMAX epilogue and k_pred_next's key reduction (q3tts_k_bgemm_q8a8_argmax): the winning column of every row.
    aq int8 [B][K], ad f32 [B][K/32], weights q int8 [N][K] / d16 f16 bits [N][K/32]; ssp [B][ntiles] or None (no row scale)."""
    lib = _abi.load_library()
    aq = np.ascontiguousarray(aq, dtype=np.int8); ad = np.ascontiguousarray(ad, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.int8); d16 = np.ascontiguousarray(d16, dtype=np.uint16)
    B, K = aq.shape
    N = q.shape[0]
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    ids = np.full(B, -1, dtype=np.int32)
    rc = lib.q3tts_k_bgemm_q8a8_argmax(device, aq.ctypes.data, ad.ctypes.data, B, K, q.ctypes.data, d16.ctypes.data, N, None if sp is None else sp.ctypes.data,
                                       0 if sp is None else sp.shape[1], d_norm, eps, ids.ctypes.data)
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_bgemm_q8a8_argmax failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return ids


def k_bgemm_q8a8(aq, ad, q, d16, ssp, d_norm, eps, epi, nw_next=None, y0=None, device=0, iters=0):
    """The decoder's GEMM in ggml's Q8_0 x Q8_0 arithmetic (q3tts_k_bgemm_q8a8): activations aq int8 [B][K] + their block scales ad [B][K/32], weights q / d16.
    ad: f32 (what the W8A8 producers store: d rounded to f16's 11-bit significand, kept in f32; yd comes back as f32) or f16 bit patterns
    (uint16: widened exactly; yd then comes back as f16 bit patterns too, exact wherever the produced scale is a normal f16)."""
    lib = _abi.load_library()
    aq = np.ascontiguousarray(aq, dtype=np.int8); ad = np.asarray(ad)
    as_f16 = ad.dtype == np.uint16
    if as_f16:
        ad = ad.view(np.float16).astype(np.float32)
    elif ad.dtype != np.float32:
        raise _abi.Q3Error(f"k_bgemm_q8a8: ad must be float32 or f16 bit patterns (uint16), got {ad.dtype}")
    ad = np.ascontiguousarray(ad)
    q = np.ascontiguousarray(q, dtype=np.int8); d16 = np.ascontiguousarray(d16, dtype=np.uint16)
    B, K = aq.shape
    N = q.shape[0]
    nout = N // 2 if epi == 2 else N
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yq = np.zeros((B, nout), dtype=np.int8); yd = np.zeros((B, nout // 32), dtype=np.float32)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    ms = C.c_float(0)
    rc = lib.q3tts_k_bgemm_q8a8(device, aq.ctypes.data, ad.ctypes.data, B, K, q.ctypes.data, d16.ctypes.data, N, None if sp is None else sp.ctypes.data,
                                0 if sp is None else sp.shape[1], d_norm, eps, epi, None if nw is None else nw.ctypes.data, y.ctypes.data, yq.ctypes.data,
                                yd.ctypes.data, sso.ctypes.data, iters, C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_bgemm_q8a8 failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    if as_f16:
        with np.errstate(over="ignore"):
            yd = np.ascontiguousarray(yd.astype(np.float16)).view(np.uint16)
    return dict(y=y, yq=yq, yd=yd, ssp_out=sso, ms=ms.value)


def k_bgemm_voc(xb, wb, epi, bias=None, col_scale=None, seg_rows=0, gap_rows=0, y0=None, want_yb=False, device=0):
    """The decoder's GEMM with the vocoder's epilogue extras (q3tts_k_bgemm_voc): returns dict(y=[B][N] f32 or None, yb=[B][N] bf16 bits or None)."""
    lib = _abi.load_library()
    xb = np.ascontiguousarray(xb, dtype=np.uint16); wb = np.ascontiguousarray(wb, dtype=np.uint16)
    B, K = xb.shape
    N = wb.shape[0]
    y = None if epi == 4 else (np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy())
    yb = np.zeros((B, N), dtype=np.uint16) if (epi == 4 or want_yb) else None
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    cs = None if col_scale is None else np.ascontiguousarray(col_scale, dtype=np.float32)
    rc = lib.q3tts_k_bgemm_voc(device, xb.ctypes.data, B, K, wb.ctypes.data, N, epi, None if b is None else b.ctypes.data, 0 if b is None else b.size,
                               None if cs is None else cs.ctypes.data, seg_rows, gap_rows, None if y is None else y.ctypes.data,
                               None if yb is None else yb.ctypes.data, 1 if want_yb else 0)
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_bgemm_voc failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return dict(y=y, yb=yb)


def k_project(x, w, bias, nw=None, device=0):
    lib = _abi.load_library()
    x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w, dtype=np.float32); b = np.ascontiguousarray(bias, dtype=np.float32)
    rows, n_in = x.shape
    n_out = w.shape[0]
    y = np.zeros((rows, n_out), dtype=np.float32)
    xb = np.zeros((rows, n_out), dtype=np.uint16); ssp = np.zeros((rows, n_out // 16), dtype=np.float32)
    nwa = None if nw is None else np.ascontiguousarray(nw, dtype=np.float32)
    rc = lib.q3tts_k_project(device, x.ctypes.data, rows, n_in, w.ctypes.data, b.ctypes.data, n_out, None if nwa is None else nwa.ctypes.data,
                             y.ctypes.data, xb.ctypes.data, ssp.ctypes.data)
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_project failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return y, xb, ssp


def k_norm_inputs(x, nw, device=0):
    lib = _abi.load_library()
    x = np.ascontiguousarray(x, dtype=np.float32); nw = np.ascontiguousarray(nw, dtype=np.float32)
    rows, d = x.shape
    xb = np.zeros((rows, d), dtype=np.uint16); ssp = np.zeros((rows, d // 16), dtype=np.float32)
    rc = lib.q3tts_k_norm_inputs(device, x.ctypes.data, rows, d, nw.ctypes.data, xb.ctypes.data, ssp.ctypes.data)
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_norm_inputs failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return xb, ssp


def k_attention(qkv, pos0, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, device=0):
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    n = qkv.shape[0]
    out = np.zeros((n, n_head * head_dim), dtype=np.float32)
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    rc = lib.q3tts_k_attention(device, _ptr(qkv, f32p), n, pos0, n_head, n_kv_head, head_dim, _ptr(qn, f32p), _ptr(kn, f32p), eps,
                               rope_theta, None if sec is None else _ptr(sec, i32p), _ptr(out, f32p))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return out


def k_attention_decode(qkv, lens, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, policy=-1, device=0):
    """q3tts_k_attention_decode: qkv holds the slots' rows back to back (sum(lens) rows); returns (out_f32, out_bf16 bits), both
    [n_slots][n_head * head_dim]: one fused decode launch per output at pos = lens[s] - 1 over a cache of n_ctx positions."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    assert qkv.shape[0] == int(ln.sum())
    out = np.zeros((ln.size, n_head * head_dim), dtype=np.float32)
    ob = np.zeros((ln.size, n_head * head_dim), dtype=np.uint16)
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    rc = lib.q3tts_k_attention_decode(device, _ptr(qkv, f32p), ln.size, _ptr(ln, i32p), n_ctx, n_head, n_kv_head, head_dim, _ptr(qn, f32p),
                                      _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), policy, _ptr(out, f32p),
                                      ob.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_decode failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return out, ob


ATTEND_KERNELS = ("k_attend<1, false>", "k_attend<2, false>", "k_attend<4, false>", "k_attend<2, true>", "k_attend<4, true>", "k_attend_gqa2",
                  "k_attend_small<2>", "k_attend_pair", "k_attend_prefill")


def k_attend_pick(fused, gqa_ratio, n_ctx, n_kv_head, n_seg=0, seg_max_n=0, seg_max_t=0):
    """q3tts_k_attend_pick (host only): the name of the kernel the attention launcher takes for a shape under the current policies, or
    None when it refuses the launch."""
    lib = _abi.load_library()
    k = C.c_int32(-2)
    rc = lib.q3tts_k_attend_pick(fused, gqa_ratio, n_ctx, n_seg, seg_max_n, seg_max_t, n_kv_head, C.byref(k))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attend_pick failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return None if k.value < 0 else ATTEND_KERNELS[k.value]


ATTEND_KERNELS_KV8 = {9: "k_attend_kv8<1, false>", 10: "k_attend_kv8<2, false>", 11: "k_attend_kv8<4, false>", 12: "k_attend_kv8<2, true>",
                      13: "k_attend_kv8<4, true>", 14: "k_attend_gqa2_kv8"}


def k_attend_pick_kv8(fused, gqa_ratio, n_ctx, n_kv_head, n_seg=0, seg_max_n=0, seg_max_t=0, want_code=False):
    """q3tts_k_attend_pick_kv8 (host only): the kernel of csrc/q3_attend_kv8.hip the launcher takes for a launch over a Q8_0 cache under the
    current policies — its name (want_code: its number 9 .. 14) — or None when the launcher refuses."""
    lib = _abi.load_library()
    k = C.c_int32(-2)
    rc = lib.q3tts_k_attend_pick_kv8(fused, gqa_ratio, n_ctx, n_seg, seg_max_n, seg_max_t, n_kv_head, C.byref(k))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attend_pick_kv8 failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    if k.value < 0:
        return None
    return k.value if want_code else ATTEND_KERNELS_KV8[k.value]


def _att_hook_cache_kv8(n_slots, n_kv_head, n_ctx, head_dim, want_cache):
    if not want_cache:
        return None, None, None, None
    q = lambda: np.zeros((n_slots, n_kv_head, n_ctx, head_dim), dtype=np.int8)
    d = lambda: np.zeros((n_slots, n_kv_head, n_ctx, head_dim // 32), dtype=np.uint16)
    return q(), q(), d(), d()


def k_attention_runs_kv8(qkv, runs, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, policy=-1, out_form=0,
                         want_cache=True, device=0):
    """q3tts_k_attention_runs_kv8: k_attention_runs over a Q8_0 cache. Returns a dict: out / scale as there, and the cache un-blocked:
    k_q / v_q int8 [run][n_kv_head][n_ctx][head_dim], k_d / v_d f16 bits [run][n_kv_head][n_ctx][head_dim / 32]."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    p0 = np.ascontiguousarray([r[0] for r in runs], dtype=np.int32)
    nn = np.ascontiguousarray([r[1] for r in runs], dtype=np.int32)
    assert qkv.shape[0] == int(p0.sum() + nn.sum())
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, _, _ = _att_hook_out(max(int(nn.sum()), 1), n_head * head_dim, out_form, len(runs), n_kv_head, n_ctx, head_dim, False)
    kq, vq, kd, vd = _att_hook_cache_kv8(len(runs), n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_runs_kv8(device, _ptr(qkv, f32p), len(runs), _ptr(nn, i32p), _ptr(p0, i32p), n_ctx, n_head, n_kv_head, head_dim,
                                        _ptr(qn, f32p), _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), policy, out_form,
                                        _dp(out), _dp(sc), _dp(kq), _dp(vq), _dp(kd), _dp(vd))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_runs_kv8 failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return dict(out=out, scale=sc, k_q=kq, v_q=vq, k_d=kd, v_d=vd)


def k_attention_decode_kv8(qkv, lens, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, policy=-1, out_form=0,
                           want_cache=True, device=0):
    """q3tts_k_attention_decode_kv8: k_attention_decode_ex (without row_indexed) over a Q8_0 cache. Returns the dict of k_attention_runs_kv8
    with out [n_slots][n_head * head_dim]."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    assert qkv.shape[0] == int(ln.sum())
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, _, _ = _att_hook_out(max(ln.size, 1), n_head * head_dim, out_form, ln.size, n_kv_head, n_ctx, head_dim, False)
    kq, vq, kd, vd = _att_hook_cache_kv8(ln.size, n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_decode_kv8(device, _ptr(qkv, f32p), ln.size, _ptr(ln, i32p), n_ctx, n_head, n_kv_head, head_dim, _ptr(qn, f32p),
                                          _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), policy, out_form,
                                          _dp(out), _dp(sc), _dp(kq), _dp(vq), _dp(kd), _dp(vd))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_decode_kv8 failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return dict(out=out, scale=sc, k_q=kq, v_q=vq, k_d=kd, v_d=vd)


def _att_hook_out(rows, nq, out_form, n_slots, n_kv_head, n_ctx, head_dim, want_cache):
    out = np.zeros((rows, nq), dtype=(np.float32, np.uint16, np.int8)[out_form] if 0 <= out_form <= 2 else np.float32)
    sc = np.zeros((rows, nq // 32), dtype=np.float32) if out_form == 2 else None
    kc = np.zeros((n_slots, n_kv_head, n_ctx, head_dim), dtype=np.uint16) if want_cache else None
    vc = np.zeros((n_slots, n_kv_head, n_ctx, head_dim), dtype=np.uint16) if want_cache else None
    return out, sc, kc, vc


def _att_hook_ret(out, sc, kc, vc):
    return dict(out=out, scale=sc, k_cache=kc, v_cache=vc)


def _dp(a):
    return None if a is None else a.ctypes.data


def k_attention_runs(qkv, runs, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, policy=-1, out_form=0,
                     want_cache=True, device=0):
    """q3tts_k_attention_runs: runs = [(pos0, n), ...], one slot each; qkv holds every run's pos0 + n rows back to back. Returns a dict:
    out [sum n][n_head * head_dim] in the form asked for (f32 / bf16 bits / int8 with `scale`), k_cache / v_cache bf16 bits
    [run][n_kv_head][n_ctx][head_dim]."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    p0 = np.ascontiguousarray([r[0] for r in runs], dtype=np.int32)
    nn = np.ascontiguousarray([r[1] for r in runs], dtype=np.int32)
    assert qkv.shape[0] == int(p0.sum() + nn.sum())
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, kc, vc = _att_hook_out(max(int(nn.sum()), 1), n_head * head_dim, out_form, len(runs), n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_runs(device, _ptr(qkv, f32p), len(runs), _ptr(nn, i32p), _ptr(p0, i32p), n_ctx, n_head, n_kv_head, head_dim,
                                    _ptr(qn, f32p), _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), policy, out_form,
                                    _dp(out), _dp(sc), _dp(kc), _dp(vc))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_runs failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return _att_hook_ret(out, sc, kc, vc)


def k_attention_decode_ex(qkv, lens, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, policy=-1,
                          row_indexed=False, out_form=0, want_cache=True, device=0):
    """q3tts_k_attention_decode_ex: k_attention_decode with one output form per call, the cache, and the Predictor's row-indexed addressing.
    Returns the dict of k_attention_runs with out [n_slots][n_head * head_dim]."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    assert qkv.shape[0] == int(ln.sum())
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, kc, vc = _att_hook_out(max(ln.size, 1), n_head * head_dim, out_form, ln.size, n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_decode_ex(device, _ptr(qkv, f32p), ln.size, _ptr(ln, i32p), n_ctx, n_head, n_kv_head, head_dim, _ptr(qn, f32p),
                                         _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), policy,
                                         1 if row_indexed else 0, out_form, _dp(out), _dp(sc), _dp(kc), _dp(vc))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_decode_ex failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return _att_hook_ret(out, sc, kc, vc)


def k_attention_pair(qkv, n_slots, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, out_form=0,
                     want_cache=True, device=0):
    """q3tts_k_attention_pair: qkv [2 * n_slots] rows in the Predictor's order (row b at position 0, row n_slots + b at position 1). Returns
    the dict of k_attention_runs with out [2 * n_slots][n_head * head_dim]."""
    lib = _abi.load_library()
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    assert qkv.shape[0] == 2 * n_slots
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, kc, vc = _att_hook_out(max(2 * n_slots, 1), n_head * head_dim, out_form, n_slots, n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_pair(device, _ptr(qkv, f32p), n_slots, n_ctx, n_head, n_kv_head, head_dim, _ptr(qn, f32p), _ptr(kn, f32p), eps,
                                    rope_theta, None if sec is None else _ptr(sec, i32p), out_form, _dp(out), _dp(sc), _dp(kc), _dp(vc))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_pair failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return _att_hook_ret(out, sc, kc, vc)


class PredStepState:
    """The arrays behind a q3tts_k_pred_step (q3tts_k_pred_next / q3tts_k_attention_gather): row b stands for slot b. keys u64
    [n_rows][n_key_parts]; active / n_frames [n_rows]; codec_q [rows_q][d_embed]; pproj_q [rows_q][d_proj]; proj_b [d_proj]; fb, px and codes
    ([n_rows][max_steps_cap][n_codebooks]) are copied here and updated in place by a call."""

    def __init__(self, q, n_codebooks, keys, active, n_frames, codec_q, pproj_q, proj_b, fb, px, codes):
        c = np.ascontiguousarray
        self.keys = c(keys, dtype=np.uint64); self.active = c(active, dtype=np.int32); self.n_frames = c(n_frames, dtype=np.int32)
        self.codec_q = c(codec_q, dtype=np.float32); self.pproj_q = c(pproj_q, dtype=np.float32); self.proj_b = c(proj_b, dtype=np.float32)
        self.fb = np.array(fb, dtype=np.float32, order="C"); self.px = np.array(px, dtype=np.float32, order="C")
        self.codes = np.array(codes, dtype=np.int32, order="C")
        n = self.keys.shape[0]
        assert self.active.shape == (n,) and self.n_frames.shape == (n,) and self.fb.shape == (n, self.codec_q.shape[1])
        assert self.px.shape == (n, self.pproj_q.shape[1]) and self.codes.shape[0] == n and self.codes.shape[2] == n_codebooks
        st = _abi.PredStep()
        st.n_rows, st.q, st.n_codebooks, st.n_key_parts, st.rows_q = n, q, n_codebooks, self.keys.shape[1], self.codec_q.shape[0]
        st.d_embed, st.d_proj, st.max_steps_cap = self.codec_q.shape[1], self.pproj_q.shape[1], self.codes.shape[1]
        for name in ("keys", "active", "n_frames", "codec_q", "pproj_q", "proj_b", "fb", "px", "codes"):
            setattr(st, name, getattr(self, name).ctypes.data)
        self.st = st


def k_pred_next(state, norm_w, device=0):
    """q3tts_k_pred_next: k_pred_next<false>(q) on a PredStepState (fb / px / codes updated in place). Returns the norm inputs it wrote for
    norm_w: (xb bf16 bits [n_rows][d_proj], ssp [n_rows][d_proj / 16])."""
    lib = _abi.load_library()
    nw = np.ascontiguousarray(norm_w, dtype=np.float32)
    n, dp = state.px.shape
    xb = np.zeros((n, dp), dtype=np.uint16); ssp = np.zeros((n, dp // 16), dtype=np.float32)
    rc = lib.q3tts_k_pred_next(device, C.byref(state.st), nw.ctypes.data, xb.ctypes.data, ssp.ctypes.data)
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pred_next failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return xb, ssp


def k_attention_gather(state, table, qkv, length, n_ctx, n_head, n_kv_head, head_dim, q_norm_w, k_norm_w, eps, rope_theta, sections, out_form=0,
                       want_cache=True, device=0):
    """q3tts_k_attention_gather: one gathering launch of k_attend_small<2> on a PredStepState (updated in place). table [rows_q + 1][ld];
    qkv: n_rows runs of `length` rows as k_attention_decode_ex takes them, of which the last row of a run is not read. Returns the dict of
    k_attention_runs with out [n_rows][n_head * head_dim]."""
    lib = _abi.load_library()
    tab = np.ascontiguousarray(table, dtype=np.float32)
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    n = state.px.shape[0]
    ld = (n_head + 2 * n_kv_head) * head_dim
    assert qkv.shape == (n * length, ld) and tab.shape == (state.codec_q.shape[0] + 1, ld)
    qn = np.ascontiguousarray(q_norm_w, dtype=np.float32)
    kn = np.ascontiguousarray(k_norm_w, dtype=np.float32)
    sec = None if sections is None else np.ascontiguousarray(sections, dtype=np.int32)
    out, sc, kc, vc = _att_hook_out(n, n_head * head_dim, out_form, n, n_kv_head, n_ctx, head_dim, want_cache)
    rc = lib.q3tts_k_attention_gather(device, C.byref(state.st), tab.ctypes.data, qkv.ctypes.data, length, n_ctx, n_head, n_kv_head, head_dim,
                                      _ptr(qn, f32p), _ptr(kn, f32p), eps, rope_theta, None if sec is None else _ptr(sec, i32p), out_form,
                                      _dp(out), _dp(sc), _dp(kc), _dp(vc))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_attention_gather failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return _att_hook_ret(out, sc, kc, vc)


def k_sample(logits, limit, temperature, top_k, top_p, r=None, device=0):
    lib = _abi.load_library()
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    n, ld = lg.shape
    out = np.zeros(n, dtype=np.int32)
    rr = None if r is None else np.ascontiguousarray(r, dtype=np.float32)
    rc = lib.q3tts_k_sample(device, _ptr(lg, f32p), n, ld, limit, temperature, top_k, top_p, None if rr is None else _ptr(rr, f32p),
                            _ptr(out, i32p))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_sample failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return out


def k_rvq(ps, pa, books, device=0):
    """q3tts_k_rvq: the clone audio encoder's split residual VQ (k_cb_transpose + k_rvq) on ps / pa [T][D] and books [ncb][CS][D], all f32;
    codes i64 [T][ncb]. pa may be None when ncb == 1."""
    lib = _abi.load_library()
    bk = np.ascontiguousarray(books, dtype=np.float32)
    s = np.ascontiguousarray(ps, dtype=np.float32)
    a = None if pa is None else np.ascontiguousarray(pa, dtype=np.float32)
    ncb, CS, D = bk.shape
    T = s.shape[0]
    assert s.shape == (T, D) and (a is None or a.shape == (T, D))
    codes = np.zeros((T, ncb), dtype=np.int64)
    rc = lib.q3tts_k_rvq(device, _ptr(s, f32p), None if a is None else _ptr(a, f32p), T, D, _ptr(bk, f32p), ncb, CS,
                         codes.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_rvq failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return codes


def k_gguf_read(path, tensor=""):
    """One tensor of a GGUF file / the array of an .npy file as f32, through the engine's own reader (host only).
    Returns (array shaped like numpy would show it, ggml type)."""
    lib = _abi.load_library()
    n = C.c_int64(0); dims = (C.c_int64 * 4)(); ty = C.c_int32(0)
    rc = lib.q3tts_k_gguf_read(os.fsencode(path), tensor.encode(), None, 0, C.byref(n), dims, C.byref(ty))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_gguf_read: {lib.q3tts_last_error(None).decode()} (status {rc})")
    out = np.zeros(n.value, dtype=np.float32)
    rc = lib.q3tts_k_gguf_read(os.fsencode(path), tensor.encode(), _ptr(out, f32p), n.value, C.byref(n), dims, C.byref(ty))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_gguf_read: {lib.q3tts_last_error(None).decode()} (status {rc})")
    shape = [int(d) for d in dims if d]
    if not str(path).endswith(".npy"):
        shape = shape[::-1]  # ggml lists the contiguous dimension first
    return out.reshape(shape), int(ty.value)


GGUF_VALUE_TYPES = ("u8", "i8", "u16", "i16", "u32", "i32", "f32", "bool", "str", "array", "u64", "i64", "f64")


def k_gguf_meta(path, key):
    """One metadata value of a GGUF file through the engine's own reader (host only): (type name, element type name, value). Numbers come
    back as floats (the hook's doubles), a string as bytes, arrays as lists of those."""
    lib = _abi.load_library()
    vt, et, n, nb = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = lib.q3tts_k_gguf_meta(os.fsencode(path), key.encode(), C.byref(vt), C.byref(et), C.byref(n), None, 0, None, 0, C.byref(nb))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_gguf_meta: {lib.q3tts_last_error(None).decode()} (status {rc})")
    vals = (C.c_double * max(1, n.value))(); buf = C.create_string_buffer(max(1, nb.value))
    rc = lib.q3tts_k_gguf_meta(os.fsencode(path), key.encode(), C.byref(vt), C.byref(et), C.byref(n), vals, n.value, buf, nb.value, C.byref(nb))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_gguf_meta: {lib.q3tts_last_error(None).decode()} (status {rc})")
    tname, ename = GGUF_VALUE_TYPES[vt.value], GGUF_VALUE_TYPES[et.value]
    raw = buf.raw[:nb.value]
    if tname == "str":
        return tname, ename, raw
    if tname != "array":
        return tname, ename, vals[0]
    if ename != "str":
        return tname, ename, list(vals[:n.value])
    out, pos = [], 0
    for _ in range(n.value):  # each element: little-endian u64 length, then its bytes
        ln = int.from_bytes(raw[pos:pos + 8], "little")
        out.append(raw[pos + 8:pos + 8 + ln])
        pos += 8 + ln
    return tname, ename, out


def config_from_model_dir(model_dir, quant=None, base=None):
    """q3tts_config_from_model_dir: a copy of `base` (default: q3tts_default_config) whose model dimensions and weights_path come from the
    files of model_dir's quant directory. The returned config owns the path buffer weights_path points into. Host only."""
    lib = _abi.load_library()
    cfg = _abi.copy_config(base) if base is not None else _abi.default_config()
    md = os.fsencode(model_dir)
    buf = C.create_string_buffer(len(md) + 16)
    err = C.create_string_buffer(1024)
    q = None if quant is None else str(quant).encode()
    rc = lib.q3tts_config_from_model_dir(md, q, C.byref(cfg), buf, len(buf), err, len(err))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_config_from_model_dir failed ({rc}): {err.value.decode('utf-8', 'replace')}")
    cfg._path_buf = buf  # weights_path points into it
    return cfg


def vocoder_config_from_file(path, base=None):
    """q3tts_vocoder_config_from_file: a copy of the vocoder block `base` (default: q3tts_default_config's) with every field the weights
    file `path` states, cross-checked against its tensor shapes. Host only."""
    lib = _abi.load_library()
    vc = _abi.VocoderConfig.from_buffer_copy(base if base is not None else _abi.default_config().vocoder)
    err = C.create_string_buffer(1024)
    rc = lib.q3tts_vocoder_config_from_file(os.fsencode(path), C.byref(vc), err, len(err))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_vocoder_config_from_file failed ({rc}): {err.value.decode('utf-8', 'replace')}")
    return vc


CLONE_FILES = ("qwen3_tts_speaker_encoder.gguf", "qwen3_tts_codec_encoder.gguf")


def clone_files_found(weights_dir):
    """q3tts_clone_files_find: (speaker file, codec file) as q3tts_clone_load would find them — in weights_dir (the quant directory), else
    in its parent; None for one that is in neither. Host only."""
    lib = _abi.load_library()
    d = os.fsencode(weights_dir)
    cap = len(d) + 64
    spk, codec = C.create_string_buffer(cap), C.create_string_buffer(cap)
    rc = lib.q3tts_clone_files_find(d, spk, codec, cap)
    if rc < 0:
        raise _abi.Q3Error(f"q3tts_clone_files_find failed ({rc}): {lib.q3tts_last_error(None).decode('utf-8', 'replace')}")
    return tuple(os.fsdecode(b.value) if b.value else None for b in (spk, codec))


def clone_config_from_dir(weights_dir, base=None):
    """q3tts_clone_config_from_dir: a copy of the clone config `base` (default: q3tts_clone_default_config's) with every field the two
    encoder files found from weights_dir state, cross-checked against their tensor shapes. Host only."""
    lib = _abi.load_library()
    if base is not None:
        cc = _abi.CloneConfig.from_buffer_copy(base)
    else:
        cc = _abi.CloneConfig()
        lib.q3tts_clone_default_config(cc)
    err = C.create_string_buffer(1024)
    rc = lib.q3tts_clone_config_from_dir(os.fsencode(weights_dir), C.byref(cc), err, len(err))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_clone_config_from_dir failed ({rc}): {err.value.decode('utf-8', 'replace')}")
    return cc


def k_clone_load_check(weights_dir):
    """q3tts_k_clone_load_check: (status, message) of the host half of q3tts_clone_load on the pair found from weights_dir. Host only."""
    lib = _abi.load_library()
    rc = lib.q3tts_k_clone_load_check(os.fsencode(weights_dir))
    return rc, ("" if rc == 0 else lib.q3tts_last_error(None).decode("utf-8", "replace"))


def k_clone_file_tensor(weights_dir, cc, comp, which):
    """q3tts_k_clone_file_tensor: the f32 array (device layout, after rounding) q3tts_clone_load would upload from the pair found from
    weights_dir for the synthetic generator's tensor id (comp, which) at the shape `cc`. Host only."""
    lib = _abi.load_library()
    n = C.c_int64(0)
    p = os.fsencode(weights_dir)
    rc = lib.q3tts_k_clone_file_tensor(p, C.byref(cc), comp, which, None, 0, C.byref(n))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_clone_file_tensor failed ({rc}): {lib.q3tts_last_error(None).decode('utf-8', 'replace')}")
    out = np.zeros(n.value, dtype=np.float32)
    rc = lib.q3tts_k_clone_file_tensor(p, C.byref(cc), comp, which, _ptr(out, f32p), out.size, C.byref(n))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_clone_file_tensor failed ({rc}): {lib.q3tts_last_error(None).decode('utf-8', 'replace')}")
    return out


def k_voc_file_tensor(path, vc, comp, which):
    """q3tts_k_voc_file_tensor: the f32 array (device layout, after rounding) the engine would upload from the vocoder file `path` for the
    synthetic generator's tensor id (comp, which) at the shape `vc`. Host only."""
    lib = _abi.load_library()
    n = C.c_int64(0)
    p = os.fsencode(path)
    rc = lib.q3tts_k_voc_file_tensor(p, C.byref(vc), comp, which, None, 0, C.byref(n))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_voc_file_tensor failed ({rc}): {lib.q3tts_last_error(None).decode('utf-8', 'replace')}")
    out = np.zeros(n.value, dtype=np.float32)
    rc = lib.q3tts_k_voc_file_tensor(p, C.byref(vc), comp, which, _ptr(out, f32p), out.size, C.byref(n))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_voc_file_tensor failed ({rc}): {lib.q3tts_last_error(None).decode('utf-8', 'replace')}")
    return out


def k_pcm_pack(src, entries, out_n, fmt=0, device=0):
    """q3tts_k_pcm_pack: src [rows][stride] f32, entries [(row, first, count, dst)] (<= 64); returns the f32 (fmt 0) or i16 (fmt 1) output
    of out_n samples (zeros outside the windows)."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(src, dtype=np.float32)
    rows, stride = src.shape
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    er, ef, ec = (np.ascontiguousarray(e[:, i], dtype=np.int32) for i in range(3))
    ed = np.ascontiguousarray(e[:, 3], dtype=np.int64)
    out = np.zeros(max(int(out_n), 1), dtype=np.int16 if fmt else np.float32)
    rc = lib.q3tts_k_pcm_pack(device, _ptr(src, f32p), rows, stride, _ptr(er, i32p), _ptr(ef, i32p), _ptr(ec, i32p),
                              ed.ctypes.data_as(C.POINTER(C.c_int64)), len(e), fmt, out.ctypes.data, int(out_n))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pcm_pack failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return out[:int(out_n)]


def k_resample_table(rate_in, rate_out):
    """q3tts_k_resample_table (host only): (L, M, H, tab [L][2H + 1] f32) of the resampler's filter for rate_in -> rate_out."""
    lib = _abi.load_library()
    L, M, H, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    tab = np.zeros(32768, dtype=np.float32)
    rc = lib.q3tts_k_resample_table(int(rate_in), int(rate_out), C.byref(L), C.byref(M), C.byref(H), _ptr(tab, f32p), tab.size, C.byref(n))
    if rc != 0:
        e = _abi.Q3Error(f"q3tts_k_resample_table failed ({rc}): {lib.q3tts_last_error(None).decode()}")
        e.status = rc
        raise e
    return L.value, M.value, H.value, tab[:n.value].reshape(L.value, 2 * H.value + 1).copy()


def k_pcm_resample(src, row_len, row_final, entries, out_n, rate_in, rate_out, fmt=0, device=0, iters=0):
    """q3tts_k_pcm_resample: src [rows][stride] f32 at rate_in with row_len[r] valid samples per row (finished or not: row_final[r]),
    entries [(row, first_out, count, dst)] (<= 64) in output samples at rate_out; returns the f32 (fmt 0) or i16 (fmt 1) output of out_n
    samples (zeros outside the windows); with iters > 0, (that, the launch's mean time in ms over iters repetitions)."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(src, dtype=np.float32)
    rows, stride = src.shape
    ms = C.c_float(0)
    rl, rf = np.ascontiguousarray(row_len, dtype=np.int32), np.ascontiguousarray(row_final, dtype=np.int32)
    if rl.shape != (rows,) or rf.shape != (rows,):
        raise ValueError("k_pcm_resample: row_len and row_final take one value per row of src")
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    er, ef, ec = (np.ascontiguousarray(e[:, i], dtype=np.int32) for i in range(3))
    ed = np.ascontiguousarray(e[:, 3], dtype=np.int64)
    out = np.zeros(max(int(out_n), 1), dtype=np.int16 if fmt else np.float32)
    rc = lib.q3tts_k_pcm_resample(device, _ptr(src, f32p), rows, stride, _ptr(rl, i32p), _ptr(rf, i32p), _ptr(er, i32p), _ptr(ef, i32p),
                                  _ptr(ec, i32p), ed.ctypes.data_as(C.POINTER(C.c_int64)), len(e), int(rate_in), int(rate_out), fmt,
                                  out.ctypes.data, int(out_n), int(iters), C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pcm_resample failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return (out[:int(out_n)], ms.value) if iters > 0 else out[:int(out_n)]


def k_tempo_counts(n, permille):
    """q3tts_k_tempo_counts (host only): (N_t(n), D_t(n)) of the time-stretch at `permille`."""
    lib = _abi.load_library()
    N, D = C.c_int64(), C.c_int64()
    rc = lib.q3tts_k_tempo_counts(int(n), int(permille), C.byref(N), C.byref(D))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_tempo_counts failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return N.value, D.value


def k_pcm_tempo(src, lens, row_final, permille, out_stride, delta_stride=0, device=0, iters=0):
    """q3tts_k_pcm_tempo: src [rows][stride] f32; lens [n_steps][rows] valid lengths (one launch per step), row_final[r]: the last step
    finishes row r. Returns (out [n_steps][rows][out_stride] f32 — the whole output rows after every step, NaN where nothing was written —,
    n_valid [n_steps][rows], delta [rows][delta_stride] i32); with iters > 0 the last step's mean launch time in ms as a fourth."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(src, dtype=np.float32)
    rows, stride = src.shape
    ln = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1, rows)
    rf = np.ascontiguousarray(row_final, dtype=np.int32)
    if rf.shape != (rows,):
        raise ValueError("k_pcm_tempo: row_final takes one value per row of src")
    steps = ln.shape[0]
    out = np.zeros((steps, rows, int(out_stride)), dtype=np.float32)
    nv = np.zeros((steps, rows), dtype=np.int32)
    dl = np.zeros((rows, max(int(delta_stride), 1)), dtype=np.int32)
    ms = C.c_float(0)
    rc = lib.q3tts_k_pcm_tempo(device, _ptr(src, f32p), rows, stride, _ptr(ln, i32p), steps, _ptr(rf, i32p), int(permille), _ptr(out, f32p),
                               int(out_stride), _ptr(nv, i32p), _ptr(dl, i32p), int(delta_stride), int(iters), C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pcm_tempo failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    dl = dl[:, :int(delta_stride)]
    return (out, nv, dl, ms.value) if iters > 0 else (out, nv, dl)


def text_split(text, target_bytes=0, max_bytes=0):
    """q3tts_text_split (host only): UTF-8 text (str or bytes) -> [(begin, end, kind)], byte ranges of the source with their break kind
    (_abi.BREAK_*); 0 selects the defaults (120 / 240 bytes)."""
    lib = _abi.load_library()
    raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    cap = 16
    err = C.create_string_buffer(256)
    while True:
        spans = (_abi.TextSpan * cap)()
        n = C.c_int32(0)
        rc = lib.q3tts_text_split(raw, len(raw), int(target_bytes), int(max_bytes), spans, cap, C.byref(n), err, len(err))
        if rc != 0 and n.value > cap:  # *n_spans carries the size needed
            cap = n.value
            continue
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_text_split failed ({rc}): {err.value.decode('utf-8', 'replace')}")
        return [(int(spans[i].begin), int(spans[i].end), int(spans[i].kind)) for i in range(n.value)]


def join_opts(trim=1, threshold=0.01, keep=480, fade=120, pause_ms=(0, 0, 150, 300, 600)):
    """A q3tts_join_opts with the header's defaults."""
    o = _abi.JoinOpts()
    o.trim, o.threshold, o.keep, o.fade = int(trim), float(threshold), int(keep), int(fade)
    o.pause_ms[:] = [int(p) for p in pause_ms]
    return o


def pcm_join(engine: "NativeEngine", clips, kinds, **opts):
    """q3tts_pcm_join: finished host clips and their break kinds -> (the joined f32 PCM, edges [n][4] = lo, hi, begin, end)."""
    return engine.pcm_join(clips, kinds, **opts)


def _long_rows(src, lens):
    src = np.ascontiguousarray(src, dtype=np.float32)
    ln = np.ascontiguousarray(lens, dtype=np.int32)
    if src.ndim != 2 or ln.shape != (src.shape[0],):
        raise ValueError("src is [rows][stride] and lens takes one value per row")
    return src, ln


def k_pcm_edges(src, lens, threshold, device=0, iters=0):
    """q3tts_k_pcm_edges: src [rows][stride] f32 with lens[r] valid samples -> edges [rows][2] = the first and last loud block of 240
    samples (INT32_MAX, -1 when none is); with iters > 0 the mean launch time in ms as a second."""
    lib = _abi.load_library()
    src, ln = _long_rows(src, lens)
    ed = np.zeros((src.shape[0], 2), dtype=np.int32)
    ms = C.c_float(0)
    rc = lib.q3tts_k_pcm_edges(device, _ptr(src, f32p), src.shape[0], src.shape[1], _ptr(ln, i32p), float(threshold), _ptr(ed, i32p), int(iters), C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pcm_edges failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return (ed, ms.value) if iters > 0 else ed


def k_pcm_join(src, lens, kinds, edges, out_cap, rate=24000, device=0, iters=0, **opts):
    """q3tts_k_pcm_join: the plan from `edges` (as k_pcm_edges gives them), the kinds and the join options, then one launch. Returns (out
    [out_cap] f32, NaN where the launch wrote nothing, plan [rows][4] = lo, hi, begin, end, N); with iters > 0 the mean launch time too."""
    lib = _abi.load_library()
    src, ln = _long_rows(src, lens)
    kd = np.ascontiguousarray(kinds, dtype=np.int32)
    ed = np.ascontiguousarray(edges, dtype=np.int32)
    if kd.shape != ln.shape or ed.shape != (ln.size, 2):
        raise ValueError("k_pcm_join: kinds takes one value per row and edges two")
    o = join_opts(**opts)
    out = np.full(int(out_cap), np.nan, dtype=np.float32)
    plan = np.zeros((ln.size, 4), dtype=np.int64)
    N, ms = C.c_int64(0), C.c_float(0)
    rc = lib.q3tts_k_pcm_join(device, _ptr(src, f32p), src.shape[0], src.shape[1], _ptr(ln, i32p), _ptr(kd, i32p), _ptr(ed, i32p), C.byref(o), int(rate),
                              _ptr(out, f32p), out.size, _ptr(plan, C.POINTER(C.c_int64)), C.byref(N), int(iters), C.byref(ms))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_pcm_join failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return (out, plan, N.value, ms.value) if iters > 0 else (out, plan, N.value)


def doc_opts(ahead=0, open=0, speed_permille=0, output_rate=0, **join):
    """q3tts_doc_opts: q3tts_doc_default_opts, then the join options given, ahead / open and the document's own speed / output rate."""
    lib = _abi.load_library()
    o = _abi.DocOpts()
    lib.q3tts_doc_default_opts(C.byref(o))
    if join:
        d = dict(trim=o.join.trim, threshold=o.join.threshold, keep=o.join.keep, fade=o.join.fade, pause_ms=list(o.join.pause_ms))
        d.update(join)
        o.join = join_opts(**d)
    o.ahead, o.open = int(ahead), int(open)
    o.speed_permille, o.output_rate = int(speed_permille), int(output_rate)
    return o


def k_doc_rules(opts, kinds, have_voice=1, have_prefix=0, engine_speed=0, engine_rate=0):
    """q3tts_k_doc_rules (host only): (status, the rule's name) for a document of these options and break kinds."""
    lib = _abi.load_library()
    kd = np.ascontiguousarray(kinds, dtype=np.int32)
    msg = C.create_string_buffer(256)
    rc = lib.q3tts_k_doc_rules(C.byref(opts) if opts is not None else None, _ptr(kd, i32p) if kd.size else None, kd.size, int(have_voice), int(have_prefix),
                               int(engine_speed), int(engine_rate), msg, 256)
    return rc, msg.value.decode()


def k_doc_plan(segs, room, state, rate=24000, **opts):
    """q3tts_k_doc_plan (host only): one boundary of the streaming join's plan. segs [n][5] = n, first, last, closed, kind; state: int64 [7],
    updated in place (zeros before the first call). Returns (pieces [k][6] = seg, src, j0, count, L, F; done [m][5] = seg, lo, hi, begin, end)."""
    lib = _abi.load_library()
    sg = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 5)
    if state.dtype != np.int64 or state.shape != (7,) or not state.flags.c_contiguous:
        raise ValueError("k_doc_plan: state is a contiguous int64 [7]")
    o = join_opts(**opts)
    i64p = C.POINTER(C.c_int64)
    cap = 2 * sg.shape[0] + 2
    pieces, done = np.zeros((cap, 6), dtype=np.int64), np.zeros((sg.shape[0] + 1, 5), dtype=np.int64)
    npc, nd = C.c_int32(0), C.c_int32(0)
    rc = lib.q3tts_k_doc_plan(C.byref(o), int(rate), _ptr(sg, i32p), sg.shape[0], int(room), _ptr(state, i64p), _ptr(pieces, i64p), cap, C.byref(npc),
                              _ptr(done, i64p), done.shape[0], C.byref(nd))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_doc_plan failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return pieces[:npc.value].copy(), done[:nd.value].copy()


def k_doc_stream(src, kinds, sched, ahead, staging, dst0=0, lag=1, fmt=0, check_rows=0, rate=24000, device=0, out_cap=None, chunk_cap=1 << 16, **opts):
    """q3tts_k_doc_stream: scan + plan + emit boundary by boundary over the rows src [rows][stride]; sched[i] lists segment i's valid length
    after every boundary at which it runs (ascending, the last one final). Returns (out f32 or i16, chunks per boundary, plan [rows][4] =
    lo, hi, begin, end, bad)."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(src, dtype=np.float32)
    kd = np.ascontiguousarray(kinds, dtype=np.int32)
    if src.ndim != 2 or kd.shape != (src.shape[0],) or len(sched) != src.shape[0]:
        raise ValueError("k_doc_stream: src is [rows][stride]; kinds and sched take one entry per row")
    sn = np.array([len(s) for s in sched], dtype=np.int32)
    sc = np.zeros((src.shape[0], max(1, int(sn.max()))), dtype=np.int32)
    for i, s in enumerate(sched):
        sc[i, :len(s)] = s
    o = join_opts(**opts)
    if out_cap is None:
        out_cap = int(sum(s[-1] for s in sched)) + (len(sched) - 1) * max(opts.get("pause_ms", (0, 0, 150, 300, 600))) * rate // 1000
    out = np.zeros(max(1, int(out_cap)), dtype=np.int16 if fmt else np.float32)
    chunks = np.zeros(int(chunk_cap), dtype=np.int64)
    plan = np.zeros((src.shape[0], 4), dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    n_out, bad, nb = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    rc = lib.q3tts_k_doc_stream(device, _ptr(src, f32p), src.shape[0], src.shape[1], _ptr(kd, i32p), _ptr(sc, i32p), _ptr(sn, i32p), sc.shape[1], C.byref(o),
                                int(rate), int(ahead), int(lag), int(staging), int(dst0), int(fmt), int(check_rows), out.ctypes.data_as(C.c_void_p),
                                int(out_cap), C.byref(n_out), _ptr(chunks, i64p), chunks.size, C.byref(nb), _ptr(plan, i64p), C.byref(bad))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_doc_stream failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    return out[:n_out.value].copy(), chunks[:nb.value].copy(), plan, bad.value


def k_doc_stream_rate(src, kinds, sched, ahead, staging, speed_permille=0, output_rate=0, ring_j=0, ring_t=0, dst0=0, lag=1, fmt=0, rate=24000,
                      device=0, out_cap=None, chunk_cap=1 << 16, delta_cap=4096, **opts):
    """q3tts_k_doc_stream_rate: k_doc_stream with a speed and / or an output rate — scan, plan, join into the ring RJ, stretch into RT,
    exit — boundary by boundary. ring_j / ring_t: the rings' capacities (0: the minimum). staging and the chunks are in output samples.
    Returns (out f32 or i16, chunks per boundary, plan [rows][4] = lo, hi, begin, end in J, bad, delta of every frame)."""
    lib = _abi.load_library()
    src = np.ascontiguousarray(src, dtype=np.float32)
    kd = np.ascontiguousarray(kinds, dtype=np.int32)
    if src.ndim != 2 or kd.shape != (src.shape[0],) or len(sched) != src.shape[0]:
        raise ValueError("k_doc_stream_rate: src is [rows][stride]; kinds and sched take one entry per row")
    sn = np.array([len(s) for s in sched], dtype=np.int32)
    sc = np.zeros((src.shape[0], max(1, int(sn.max()))), dtype=np.int32)
    for i, s in enumerate(sched):
        sc[i, :len(s)] = s
    o = join_opts(**opts)
    if out_cap is None:
        nj = int(sum(s[-1] for s in sched)) + (len(sched) - 1) * max(opts.get("pause_ms", (0, 0, 150, 300, 600))) * rate // 1000
        if speed_permille not in (0, 1000):
            nj = -(-nj * 1000 // int(speed_permille))
        if output_rate not in (0, rate):
            nj = -(-nj * int(output_rate) // int(rate))
        out_cap = nj + 64
    out = np.zeros(max(1, int(out_cap)), dtype=np.int16 if fmt else np.float32)
    chunks = np.zeros(int(chunk_cap), dtype=np.int64)
    plan = np.zeros((src.shape[0], 4), dtype=np.int64)
    delta = np.zeros(max(1, int(delta_cap)), dtype=np.int32)
    i64p = C.POINTER(C.c_int64)
    n_out, bad, nb, nf = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
    rc = lib.q3tts_k_doc_stream_rate(device, _ptr(src, f32p), src.shape[0], src.shape[1], _ptr(kd, i32p), _ptr(sc, i32p), _ptr(sn, i32p), sc.shape[1],
                                     C.byref(o), int(rate), int(ahead), int(lag), int(staging), int(dst0), int(fmt), 0, out.ctypes.data_as(C.c_void_p),
                                     int(out_cap), C.byref(n_out), _ptr(chunks, i64p), chunks.size, C.byref(nb), _ptr(plan, i64p), C.byref(bad),
                                     int(speed_permille), int(output_rate), int(ring_j), int(ring_t), _ptr(delta, i32p), int(delta_cap), C.byref(nf))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_doc_stream_rate failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    if nf.value > delta_cap:
        raise _abi.Q3Error("k_doc_stream_rate: more frames than delta_cap")
    return out[:n_out.value].copy(), chunks[:nb.value].copy(), plan, bad.value, delta[:nf.value].copy()


def k_doc_ring_plan(state, want, fin_if_all, room_out, speed_permille=0, output_rate=0, ring_j=0, ring_t=0, rate=24000):
    """q3tts_k_doc_ring_plan (host only): one boundary of a rated document's flow control. state: int64 [4] = samples joined, J whole,
    frames decided, outputs delivered, updated in place. Returns a dict of the step's counts and the two minimum capacities."""
    lib = _abi.load_library()
    if state.dtype != np.int64 or state.shape != (4,) or not state.flags.c_contiguous:
        raise ValueError("k_doc_ring_plan: state is a contiguous int64 [4]")
    out = np.zeros(13, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    rc = lib.q3tts_k_doc_ring_plan(int(speed_permille), int(rate), int(output_rate), int(ring_j), int(ring_t), _ptr(state, i64p), int(want), int(fin_if_all),
                                   int(room_out), _ptr(out, i64p))
    if rc != 0:
        raise _abi.Q3Error(f"q3tts_k_doc_ring_plan failed ({rc}): {lib.q3tts_last_error(None).decode()}")
    names = ("room", "joined", "k_from", "k_to", "nt", "nx", "fin_x", "first", "count", "all_out", "min_j", "min_t", "pending")
    return {k: int(v) for k, v in zip(names, out)}


def k_rng_f32(seed, n):
    lib = _abi.load_library()
    out = np.zeros(n, dtype=np.float32)
    lib.q3tts_k_rng_f32(seed, n, _ptr(out, f32p))
    return out


def stream_chunks(engine: "NativeEngine", **kw):
    """Generator over the streaming C ABI (q3tts_stream_begin / _poll / _end): yields (pcm_chunk, is_final); the final
    StopIteration value is the GenResult with all codes and PCM."""
    r, keep = engine.make_request(**kw)
    h = C.c_void_p()
    engine._check(engine.lib.q3tts_stream_begin(engine.h, C.byref(r), C.byref(h)), "q3tts_stream_begin")
    chunk, n, fin = f32p(), C.c_int32(), C.c_int32()
    try:
        while True:
            engine._check(engine.lib.q3tts_stream_poll(h, C.byref(chunk), C.byref(n), C.byref(fin)), "q3tts_stream_poll")
            if n.value > 0:
                yield np.ctypeslib.as_array(chunk, shape=(n.value,)).copy(), bool(fin.value)
            if fin.value:
                break
    finally:
        res = _abi.Result()
        engine._check(engine.lib.q3tts_stream_end(h, C.byref(res)), "q3tts_stream_end")
        engine.last_stream_result = engine._unpack(res)


class NativeTokenizer:
    """The C++ byte-level BPE reader (csrc/q3_tokenizer.cpp) behind Tokenizer::load / encode / decode of the reference
    (src/utils/tokenizer.rs). Host only."""

    def __init__(self, tokenizer_json_path):
        self.lib = _abi.load_library()
        self.h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self.lib.q3tts_tokenizer_load(os.fsencode(str(tokenizer_json_path)), C.byref(self.h), err, len(err))
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_tokenizer_load failed ({rc}): {err.value.decode('utf-8', 'replace')}")

    def close(self):
        if self.h:
            self.lib.q3tts_tokenizer_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def vocab_size(self):
        return int(self.lib.q3tts_tokenizer_vocab_size(self.h))

    def encode(self, text):
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        cap = max(16, len(raw) + 8)
        ids = np.zeros(cap, dtype=np.uint32)
        n = C.c_int32(0)
        err = C.create_string_buffer(512)
        rc = self.lib.q3tts_tokenizer_encode(self.h, raw, len(raw), _ptr(ids, u32p), cap, C.byref(n), err, len(err))
        if rc != 0 and n.value > cap:  # NFC can lengthen the text (composition exclusions): *n_ids carries the size needed
            cap = n.value
            ids = np.zeros(cap, dtype=np.uint32)
            rc = self.lib.q3tts_tokenizer_encode(self.h, raw, len(raw), _ptr(ids, u32p), cap, C.byref(n), err, len(err))
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_tokenizer_encode failed ({rc}): {err.value.decode('utf-8', 'replace')}")
        return ids[:n.value].copy()

    def decode(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        cap = 64 + 64 * a.size
        out = C.create_string_buffer(cap)
        n = C.c_int64(0)
        err = C.create_string_buffer(512)
        rc = self.lib.q3tts_tokenizer_decode(self.h, _ptr(a, u32p), a.size, out, cap, C.byref(n), err, len(err))
        if rc != 0:
            raise _abi.Q3Error(f"q3tts_tokenizer_decode failed ({rc}): {err.value.decode('utf-8', 'replace')}")
        return out.raw[:n.value].decode("utf-8", "replace")
