"""Host-side mirror of the reference crate's public API (names, argument meaning and error behaviour), over the C ABI.

Reference surface (src/lib.rs:11-20): TtsEngine, SamplerConfig, VoiceFile, AudioSample, PromptBuilder, cleanup().
The reference is Rust; Rust is not available in this image, so the host side above the C ABI is mirrored here in
Python for the tests and in `rust/` as (uncompiled) binding source — see INTEGRATION.md.
"""
import ctypes as C
import json
import os
import struct
import wave
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _abi, native

LANG_ID_CHINESE = 2055  # hard-coded in the reference: src/tts/engine.rs:267,407,425


@dataclass
class SamplerConfig:
    """src/tts/engine.rs:14-45 — defaults 0.7 / 40 / 0.9 / None."""
    temperature: float = 0.7
    top_k: int = 40
    top_p: float = 0.9
    seed: Optional[int] = None


@dataclass
class VoiceFile:
    """src/utils/voice_file.rs:5-62 — serde JSON; `spk_emb` is an alias of `speaker_embedding`; unknown keys ignored."""
    ref_text: str = ""
    audio_codes: List[int] = field(default_factory=list)
    speaker_embedding: List[float] = field(default_factory=list)
    name: Optional[str] = None
    gender: Optional[str] = None
    age: Optional[str] = None
    description: Optional[str] = None

    @staticmethod
    def new(ref_text, audio_codes, speaker_embedding):
        return VoiceFile(ref_text, list(audio_codes), list(speaker_embedding))

    def with_metadata(self, name=None, gender=None, age=None, description=None):
        self.name, self.gender, self.age, self.description = name, gender, age, description
        return self

    @staticmethod
    def load(path):
        with open(path, "r", encoding="utf-8") as f:
            d = json.load(f)
        emb = d.get("speaker_embedding", d.get("spk_emb"))
        if emb is None:
            raise ValueError("missing field `speaker_embedding`")  # serde: the only non-default, non-Option field
        return VoiceFile(d.get("ref_text", ""), list(d.get("audio_codes", [])), list(emb), d.get("name"), d.get("gender"),
                         d.get("age"), d.get("description"))

    def save(self, path):
        with open(path, "w", encoding="utf-8") as f:
            json.dump({"ref_text": self.ref_text, "audio_codes": self.audio_codes, "speaker_embedding": self.speaker_embedding,
                       "name": self.name, "gender": self.gender, "age": self.age, "description": self.description}, f, indent=2)


@dataclass
class AudioSample:
    """src/utils/audio.rs:4-46 — mono 24 kHz f32 container; WAV i/o is 16-bit."""
    samples: np.ndarray
    sample_rate: int = 24000
    channels: int = 1

    @staticmethod
    def load_wav(path):
        with wave.open(str(path), "rb") as w:
            if w.getsampwidth() != 2:
                raise ValueError("load_wav reads 16-bit PCM only (src/utils/audio.rs:14-17)")
            raw = w.readframes(w.getnframes())
            data = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
            return AudioSample(data, w.getframerate(), w.getnchannels())

    def save_wav(self, path):
        amp = np.clip(np.asarray(self.samples, dtype=np.float32) * np.float32(32767.0), -32768.0, 32767.0)
        pcm = np.trunc(amp).astype("<i2")  # Rust `as i16` truncates toward zero (src/utils/audio.rs:35-37)
        with wave.open(str(path), "wb") as w:
            w.setnchannels(self.channels)
            w.setsampwidth(2)
            w.setframerate(self.sample_rate)
            w.writeframes(pcm.tobytes())

    def duration(self):
        return len(self.samples) / float(self.sample_rate)


# ref-audio cache `TTSC` v1 (src/utils/cache.rs:5-67): magic, u32 version, usize n + i64 codes, usize n + f32 emb
def save_cache(path, codes: Sequence[int], emb: Sequence[float]):
    with open(path, "wb") as f:
        f.write(b"TTSC" + struct.pack("<I", 1))
        f.write(struct.pack("<Q", len(codes)) + np.asarray(codes, dtype="<i8").tobytes())
        f.write(struct.pack("<Q", len(emb)) + np.asarray(emb, dtype="<f4").tobytes())


def load_cache(path):
    with open(path, "rb") as f:
        if f.read(4) != b"TTSC":
            raise ValueError("Invalid magic bytes")
        if struct.unpack("<I", f.read(4))[0] != 1:
            raise ValueError("Unsupported version")
        n = struct.unpack("<Q", f.read(8))[0]
        codes = np.frombuffer(f.read(8 * n), dtype="<i8").tolist()
        m = struct.unpack("<Q", f.read(8))[0]
        emb = np.frombuffer(f.read(4 * m), dtype="<f4").tolist()
    return codes, emb


def load_tokenizer(model_dir):
    """Tokenizer::load(model_dir) (src/utils/tokenizer.rs:9-15): model_dir/tokenizer/tokenizer.json through the C++ byte-level
    BPE reader of the library (q3tts_tokenizer_*); None when the file does not exist (token ids are then the input)."""
    tj = os.path.join(model_dir, "tokenizer", "tokenizer.json")
    return native.NativeTokenizer(tj) if os.path.exists(tj) else None


class TtsEngine:
    """src/tts/engine.rs:53-72 — the engine owns weights, contexts and speakers; one utterance at a time per call
    (`&mut self`), or a list through `generate_batch_with_voice` (continuous batching, an extension)."""

    def __init__(self, cfg, tokenizer=None):
        self._native = native.NativeEngine(cfg)
        self.cfg = cfg
        self.tokenizer = tokenizer
        self.speakers = {}
        self.max_steps = min(512, cfg.max_steps_cap)  # src/tts/engine.rs:152
        self.sampler_config = SamplerConfig()

    @classmethod
    def new(cls, model_dir: Optional[str] = None, quant: str = "none", config=None, max_batch: Optional[int] = None,
            kv_cache: Optional[str] = None):
        """TtsEngine::new(model_dir, quant) (src/tts/engine.rs:84-169). With no config the model's shape comes from the GGUF files of the
        quant directory (q3tts_config_from_model_dir), whatever member of the family it holds; a config given by the caller is used as it
        is (its shapes must match the files) and is not modified. The vocoder's trained weights and shape come the same way from
        qwen3_tts_vocoder.gguf in the quant directory or in model_dir (vocoder_is_synthetic tells whether there was one). The voice-clone
        encoders are loaded when qwen3_tts_speaker_encoder.gguf and qwen3_tts_codec_encoder.gguf are both found the same way, as the
        reference loads its ONNX pair (src/tts/engine.rs:105-119); with neither nothing is loaded (load_clone_encoders gives the synthetic
        ones), with exactly one, or a pair whose embedding width or codebooks are not the model's, this raises. There is no network here: with no weight container under model_dir the
        engine uses seeded synthetic weights of the configured (default: 1.7B) shape. max_batch (1..256): the engine's slot count, in
        place of the config's (include/q3tts.h states the memory per slot; 256 slots of the 1.7B shape need n_ctx <= 1024 or so).
        kv_cache: None — a given config's own kv_q8_0 is kept (0, bf16, everywhere else); "bf16" — the Talker's K/V cache in bf16, whatever
        the config says; "q8_0" — ggml Q8_0 blocks
        (q3tts_engine_config.kv_q8_0 = 1: 0.53 of the memory; the results are not the bf16 cache's). Anything else: ValueError."""
        if kv_cache not in (None, "bf16", "q8_0"):
            raise ValueError(f"kv_cache must be None, 'bf16' or 'q8_0', not {kv_cache!r}")
        wdir = None
        if model_dir:
            quant_dir = {"q5_k_m": "gguf_q5_k_m", "q8_0": "gguf_q8_0"}.get(quant, "gguf")  # src/tts/engine.rs:91-95
            wdir = os.path.join(model_dir, quant_dir)
            if not os.path.exists(os.path.join(wdir, "qwen3_tts_talker.gguf")):  # :121-122; absent -> synthetic weights (no downloader here)
                wdir = None
        if config is not None:
            cfg = _abi.copy_config(config)
            if wdir:
                cfg.weights_path = wdir.encode()
        elif wdir:
            cfg = native.config_from_model_dir(model_dir, quant)
        else:
            cfg = _abi.default_config()
        if quant == "q8_0" and not cfg.talker_q8_0:
            cfg.talker_q8_0 = 2   # the gguf_q8_0 directory is multiplied as llama.cpp multiplies it: Q8_0 x Q8_0 (W8A8)
        if kv_cache is not None:
            cfg.kv_q8_0 = 1 if kv_cache == "q8_0" else 0
        if max_batch is not None:
            cfg.max_batch = int(max_batch)
        tok = load_tokenizer(model_dir) if model_dir else None
        clone_files = native.clone_files_found(wdir) if wdir else (None, None)
        if (clone_files[0] is None) != (clone_files[1] is None):
            missing = native.CLONE_FILES[0 if clone_files[0] is None else 1]
            raise _abi.Q3Error(f"{missing} not found in {wdir} or in {model_dir}: the clone encoders need both files "
                               f"(found {clone_files[0] or clone_files[1]})")
        eng = cls(cfg, tok)
        if clone_files[0] is not None:
            try:
                eng._native.clone_load(wdir)
                cc, m = eng._native.clone_cfg, cfg.model
                for what, have, want in (("speaker embedding width (embedding_length)", cc.se_dim, m.d_embed),
                                         ("n_codebooks", cc.ae_n_codebooks, m.n_codebooks),
                                         ("codebook_size", cc.ae_codebook_size, m.codebook_size)):
                    if have != want:
                        raise _abi.Q3Error(f"clone encoder files {clone_files[0]}, {clone_files[1]}: {what} = {have}, the model has {want}")
            except Exception:
                eng.close()
                raise
        for d in ([os.path.join(model_dir, "preset_speakers")] if model_dir else []) + ["speakers"]:  # :156-166
            if os.path.isdir(d):
                eng.load_speakers(d)
                break
        return eng

    def close(self):
        self._native.close()

    @property
    def vocoder_is_synthetic(self) -> bool:
        """True when the vocoder's weights are the seeded synthetic ones (no qwen3_tts_vocoder.gguf beside the model): the PCM is then the
        output of random filters, not speech. False with trained weights from the file. Meaningless without a vocoder (False)."""
        return self._native.vocoder_source == 1

    @property
    def clone_is_synthetic(self) -> bool:
        """True when the clone encoders' weights are the seeded synthetic ones (load_clone_encoders): cloned voices are then the output of
        random filters. False with trained weights from the two encoder files, and before any encoders are loaded."""
        return self._native.clone_source == 1

    def set_max_steps(self, steps: int):
        self.max_steps = steps

    def set_language(self, lang_id):
        """the reference hard-codes lang_id = 2055 (Chinese) at src/tts/engine.rs:267,407,425; None selects the
        no-language control block (NOTHINK variant, src/tts/prompt.rs:180-204)."""
        self.lang_id = lang_id

    def set_sampler_config(self, config: SamplerConfig):
        self.sampler_config = config

    def get_sampler_config(self) -> SamplerConfig:
        return self.sampler_config

    # The two controls below have no counterpart in the reference, whose Predictor is greedy (src/tts/engine.rs:470) and which applies no
    # penalty; the defaults keep that behaviour. They apply to requests admitted after the call.
    def set_predictor_sampler_config(self, config: SamplerConfig):
        """Sampler of the 15 residual codes of every frame (temperature 0 = greedy, the default). config.seed is ignored: the Predictor's
        draws are derived from each request's own seed."""
        self._native.set_predictor_sampler(config.temperature, config.top_k, config.top_p)

    def get_predictor_sampler_config(self) -> SamplerConfig:
        t, k, p = self._native.predictor_sampler()
        return SamplerConfig(temperature=t, top_k=k, top_p=p, seed=None)

    def set_repetition_penalty(self, p: float):
        """Repetition penalty on the Talker's code-0 logits over the codes generated so far; 1.0 = off (the default)."""
        self._native.set_repetition_penalty(p)

    def get_repetition_penalty(self) -> float:
        return self._native.repetition_penalty()

    def set_output_sample_rate(self, rate: int):
        """Sample rate of every AudioSample and stream chunk from now on (8000 for telephony, 16000, 48000, ...), resampled on the device
        (DESIGN.md §19); 0 or the vocoder's own 24000 = off, the default. The reference emits 24 kHz only."""
        self._native.set_output_rate(rate)

    def get_output_sample_rate(self) -> int:
        return self._native.get_output_rate() or self.cfg.vocoder.sample_rate

    def set_speed(self, speed: float):
        """Speaking rate of every AudioSample, stream chunk and session chunk from now on: 1.25 = a quarter faster, 0.5 .. 2.0, the pitch
        kept (a time-stretch on the device); 1.0 (or 0) = off, the default. The engine keeps it in per mille. The reference
        has no such control."""
        self._native.set_speed(int(round(float(speed) * 1000.0)))

    def get_speed(self) -> float:
        return (self._native.get_speed() or 1000) / 1000.0

    def load_speakers(self, speakers_dir):  # src/tts/engine.rs:187-208 (files that fail to parse are skipped)
        for fn in sorted(os.listdir(speakers_dir)):
            if fn.endswith(".json"):
                try:
                    self.speakers[os.path.splitext(fn)[0]] = VoiceFile.load(os.path.join(speakers_dir, fn))
                except Exception:
                    pass

    def get_speaker(self, id_or_name: str) -> VoiceFile:  # src/tts/engine.rs:211-231
        if id_or_name in self.speakers:
            return self.speakers[id_or_name]
        for v in self.speakers.values():
            if v.name == id_or_name:
                return v
        if "vivian" in self.speakers:
            return self.speakers["vivian"]
        if not self.speakers:
            raise RuntimeError("No speakers loaded in engine!")
        return next(iter(self.speakers.values()))

    def _encode(self, text: Union[str, Sequence[int]]):
        if isinstance(text, str):
            if self.tokenizer is None:
                raise _abi.Q3Error("no tokenizer.json available: pass token ids instead of text")
            return np.asarray(self.tokenizer.encode(text), dtype=np.uint32)  # src/utils/tokenizer.rs:17-25 (add_special_tokens = false)
        return np.asarray(text, dtype=np.uint32)

    def _lang(self):
        return getattr(self, "lang_id", LANG_ID_CHINESE)

    def _desc(self, text, voice: VoiceFile, instruct, part="whole"):
        ids = None if part == "voice" else self._encode(text)
        if part == "text":  # behind a voice prefix: the voice part is the prefix's
            return native.make_prompt_desc(ids, part="text")
        ins = None if instruct is None else self._encode(instruct)
        emb = np.asarray(voice.speaker_embedding, dtype=np.float32)
        if emb.size != self.cfg.model.d_embed:
            raise _abi.Q3Error(f"speaker_embedding has {emb.size} values, expected {self.cfg.model.d_embed}")
        if len(voice.audio_codes) == 0:  # src/tts/engine.rs:398-412: x-vector-only prompt
            return native.make_prompt_desc(ids, spk_emb=emb, lang_id=self._lang(), instruct_ids=ins, part=part)
        ref_ids = self._encode(voice.ref_text)  # :414-427: ICL clone prompt
        return native.make_prompt_desc(ids, spk_emb=emb, lang_id=self._lang(), instruct_ids=ins,
                                       ref_codes=np.asarray(voice.audio_codes, dtype=np.int32), ref_text_ids=ref_ids, part=part)

    def _prefix_key(self, voice, instruct):
        return id(voice), None if instruct is None else tuple(int(i) for i in self._encode(instruct)), self._lang()

    def voice_prefix(self, voice: VoiceFile, instruct=None):
        """A voice prefix (an extension: the reference rebuilds the whole prompt for every call): the Talker runs the voice part of the
        prompt — instruct, language, speaker and, for a cloned voice, its reference text and frames — once and keeps its K/V on the
        device. Pass it as prefix= with the same voice and instruct: the audio is bit-identical to a call without it. Close it (or use it
        as a context manager) when the voice is no longer needed."""
        desc, keep = self._desc(None, voice, instruct, part="voice")
        x = self._native.create_prefix(desc=desc)
        x.voice_key = self._prefix_key(voice, instruct)
        return x

    def _check_prefix(self, prefix, voice, instruct):
        if getattr(prefix, "voice_key", None) != self._prefix_key(voice, instruct):
            raise ValueError("prefix= was not made by voice_prefix() from this voice, instruct and language")

    def generate_with_voice(self, text, voice: VoiceFile, instruct=None, *, prefix=None) -> AudioSample:
        """src/tts/engine.rs:390-435. prefix: a voice_prefix(voice, instruct) of this engine (same audio, the voice rows are not run again)."""
        return self.generate_batch_with_voice([text], [voice], [instruct], prefix=prefix)[0]

    def generate_batch_with_voice(self, texts, voices, instructs=None, seeds=None, *, prefix=None):
        sc = self.sampler_config
        reqs, keep = [], []
        for i, (t, v) in enumerate(zip(texts, voices)):
            ins = None if instructs is None else instructs[i]
            if prefix is not None:
                self._check_prefix(prefix, v, ins)
            desc, k = self._desc(t, v, ins, part="whole" if prefix is None else "text")
            keep.append(k)
            seed = sc.seed if seeds is None else seeds[i]
            reqs.append(dict(desc=desc, temperature=sc.temperature, top_k=sc.top_k, top_p=sc.top_p, seed=seed, max_steps=self.max_steps,
                             want_pcm=1, prefix=prefix))
        outs = self._native.generate_batch(reqs)
        for o in outs:
            if o.status != 0:
                raise _abi.Q3Error(f"generation failed with status {o.status}")
        return [AudioSample(o.pcm, o.sample_rate, 1) for o in outs]

    def generate_long(self, text, voice: VoiceFile, instruct=None, *, prefix=None, seed=None, speed=None, sample_rate=None,
                      target_bytes=0, max_bytes=0, **join_opts):
        """A document of any length in one voice (an extension: the reference's generate_with_voice takes one text and truncates it at
        max_steps). The text is split at paragraphs, sentences and, where a sentence is too long, clauses
        (native.text_split); every span is encoded on its own and runs as a segment of one continuous batch behind a voice prefix; the
        segments' PCM is trimmed, faded and joined with pauses on the device and crosses to the host once. Returns (AudioSample,
        segments), segments a list of (text_slice, t_begin_s, t_end_s, hit_eos): where each piece of text landed in the audio (a segment
        with hit_eos False ran into max_steps). speed / sample_rate default to the engine's set_speed / set_output_sample_rate values,
        which are cleared around the call and restored. join_opts: trim, threshold, keep, fade, pause_ms (include/q3tts.h)."""
        if not isinstance(text, str):
            raise TypeError("generate_long takes the text as a str: it is split before it is encoded")
        raw = text.encode("utf-8")
        spans = native.text_split(raw, target_bytes, max_bytes)
        if not spans:
            raise ValueError("generate_long: the text holds nothing speakable")
        pieces = [raw[b:e].decode("utf-8") for b, e, _ in spans]
        segs = [(self._encode(p), k) for p, (_, _, k) in zip(pieces, spans)]
        sc = self.sampler_config
        if prefix is not None:
            self._check_prefix(prefix, voice, instruct)
            vdesc, keep = None, None
        else:
            vdesc, keep = self._desc(None, voice, instruct, part="voice")
        eng_speed, eng_rate = self._native.get_speed(), self._native.get_output_rate()
        permille = eng_speed if speed is None else int(round(float(speed) * 1000.0))
        rate = eng_rate if sample_rate is None else int(sample_rate)
        self._native.set_speed(0)
        self._native.set_output_rate(0)
        try:
            out = self._native.generate_long(segs, voice=vdesc, prefix=prefix, speed_permille=permille, output_rate=rate, join=join_opts,
                                             temperature=sc.temperature, top_k=sc.top_k, top_p=sc.top_p,
                                             seed=sc.seed if seed is None else seed, max_steps=self.max_steps)
        finally:
            self._native.set_output_rate(eng_rate)
            self._native.set_speed(eng_speed)
        r = float(out.sample_rate)
        table = [(p, f["out_begin"] / r, f["out_end"] / r, bool(f["hit_eos"])) for p, f in zip(pieces, out.info)]
        return AudioSample(out.pcm, out.sample_rate, 1), table

    def stream_long(self, text_or_pieces, voice: VoiceFile, instruct=None, *, prefix=None, seed=None, pause_ms=None, ahead=None,
                    speed=None, sample_rate=None, target_bytes=0, max_bytes=0, **join_opts):
        """generate_long's streaming twin (an extension; include/q3tts.h, "documents in a session"): the document plays
        while it is synthesised. A str is split as generate_long splits it and submitted whole; an iterator of strings (a language
        model still writing) is split piece by piece and appended as it arrives from a helper thread, each piece ending a paragraph.
        Yields (f32 chunk, segments_done): segments_done lists (text_slice, t_begin_s, t_end_s, hit_eos) for the segments that this
        chunk completed; a chunk is yielded as soon as the segment events of its boundary are taken (they arrive with it), not when
        the next chunk comes. The chunks joined are generate_long's audio for the same segments, speed and sample_rate, bit for bit.
        speed (a factor, 0.5 .. 2.0) / sample_rate (Hz) are the document's own, as generate_long names them; the times in segments_done
        are then in the stretched, resampled audio. The call is refused while the engine itself has a speed or an output rate set.
        ahead: how many segments may run in front of the one being delivered (default 8). join_opts / pause_ms: as generate_long."""
        import threading
        sc = self.sampler_config
        if prefix is not None:
            self._check_prefix(prefix, voice, instruct)
            vdesc, keep = None, None
        else:
            vdesc, keep = self._desc(None, voice, instruct, part="voice")
        if pause_ms is not None:
            join_opts["pause_ms"] = tuple(pause_ms)

        def split(text, last_kind=None):
            raw = text.encode("utf-8")
            spans = native.text_split(raw, target_bytes, max_bytes)
            pieces = [raw[b:e].decode("utf-8") for b, e, _ in spans]
            kinds = [k for _, _, k in spans]
            if kinds and last_kind is not None:
                kinds[-1] = last_kind
            return pieces, [(self._encode(p), k) for p, k in zip(pieces, kinds)]

        whole = isinstance(text_or_pieces, str)
        texts, first = [], []
        it = iter(()) if whole else iter(text_or_pieces)
        if whole:
            texts, first = split(text_or_pieces)
            if not first:
                raise ValueError("stream_long: the text holds nothing speakable")
        kw = dict(temperature=sc.temperature, top_k=sc.top_k, top_p=sc.top_p, seed=sc.seed if seed is None else seed, max_steps=self.max_steps)
        permille = 0 if speed is None else int(round(float(speed) * 1000.0))
        out_rate = 0 if sample_rate is None else int(sample_rate)
        rate = float(out_rate or self.cfg.vocoder.sample_rate)
        with native.NativeSession(self._native) as sess:
            did = sess.submit_document(first, voice=vdesc, prefix=prefix, join=join_opts, ahead=ahead or 0, open=not whole,
                                       speed_permille=permille, output_rate=out_rate, **kw)
            failure = []
            gate, live = threading.Lock(), [True]  # the feeder touches the session only while the consumer is inside this block

            def feed():
                try:
                    for piece in it:
                        p, segs = split(piece, _abi.BREAK_PARAGRAPH)
                        with gate:
                            if not live[0]:
                                return
                            if segs:
                                texts.extend(p)   # (before the append: a SEGMENT event finds its text)
                                sess.append_document(did, segs)
                    with gate:
                        if live[0]:
                            sess.append_document(did, [], close=True)
                except Exception as ex:  # the iterator failed, or the document ended meanwhile
                    failure.append(ex)
                    with gate:
                        if live[0]:
                            try:
                                sess.cancel(did)
                            except _abi.Q3Error:
                                pass
            th = threading.Thread(target=feed, daemon=True) if not whole else None
            if th is not None:
                th.start()
            try:
                # A boundary's events (the chunk, then the segments it completed, then DONE) reach the queue together: behind a chunk the
                # segments are taken without waiting, and the chunk goes out at once, not when the next one arrives
                ev, ended = None, False
                while not ended and (ev is not None or sess.open_ids):
                    if ev is None:
                        ev = sess.next(-1)
                    rid, kind, pcm, is_final, res = ev
                    ev = None
                    if rid != did:
                        continue
                    if kind == _abi.EV_CHUNK:
                        done = []
                        while True:
                            ev = sess.next(0)
                            if ev is None or ev[0] != did or ev[1] != _abi.EV_SEGMENT:
                                break
                            seg = ev[4].segment
                            f = sess.document_info(did)[0][seg]
                            done.append((texts[seg], f["out_begin"] / rate, f["out_end"] / rate, bool(f["hit_eos"])))
                        yield pcm, done
                    elif kind == _abi.EV_SEGMENT:   # (not behind a chunk of its own: cannot happen; kept out of the audio)
                        continue
                    elif kind == _abi.EV_DONE:
                        ended = True
                    else:
                        raise _abi.Q3Error(f"stream_long failed with status {res.status if res is not None else kind}" +
                                           (f": {failure[0]}" if failure else ""))
            finally:
                with gate:   # (also when the consumer stops early: the feeder ends at its next piece, the session closes below)
                    live[0] = False

    def stream_batch_with_voice(self, texts, voices, instructs=None, seeds=None, *, prefix=None, realtime_lead_s=None):
        """The streaming twin of generate_batch_with_voice: every utterance runs through one session (continuous batching over the
        engine's slots) and its 4-frame chunks are yielded as they are produced, as (index, f32 chunk, is_final); chunks of different
        utterances interleave, each utterance's come in order and its last has is_final = True.
        prefix="auto" (opt-in; the same chunks, bit for bit): within this call the first utterance of each (voice, instruct) pair is
        submitted keep-voice — its own prefill leaves the voice part's K/V behind as a prefix — and the later ones name that prefix while
        it is still pending, so the voice rows run once per pair. The prefixes are released before the call ends.
        realtime_lead_s (the same chunks, bit for bit): every request is submitted paced and granted frames by the wall clock, so that
        the audio delivered for it stays at most that many seconds (never less than one 4-frame chunk) ahead of a listener whose
        playback starts at the request's first chunk. A convenience over NativeSession.grant for consumers that play what they receive;
        a keep-voice request of prefix="auto" (the first utterance of each voice) is not paced: the C ABI has no paced keep-voice submission."""
        import time
        sc = self.sampler_config
        v = self.cfg.vocoder
        spf = int(np.prod([v.upsample_ratios[i] for i in range(v.n_upsample)] + [v.dec_rates[i] for i in range(v.n_dec_blocks)]))
        frame_s = spf / float(v.sample_rate)
        lead = None if realtime_lead_s is None else max(float(realtime_lead_s), 0.0)
        credit0 = None if lead is None else max(4, int(lead / frame_s) // 4 * 4)
        granted, started = {}, {}  # paced ids: frames of credit so far; the wall clock of the first chunk
        auto = isinstance(prefix, str)
        if auto and prefix != "auto":
            raise ValueError('prefix= is None, a voice_prefix() handle or "auto"')
        with native.NativeSession(self._native) as sess:
            index, made = {}, {}
            try:
                for i, (t, v) in enumerate(zip(texts, voices)):
                    ins = None if instructs is None else instructs[i]
                    seed = sc.seed if seeds is None else seeds[i]
                    kw = dict(temperature=sc.temperature, top_k=sc.top_k, top_p=sc.top_p, seed=seed, max_steps=self.max_steps)
                    if auto:
                        key = self._prefix_key(v, ins)
                        if key not in made:
                            desc, keep = self._desc(t, v, ins, part="whole")
                            rid, made[key] = sess.submit(desc=desc, keep_voice=True, **kw)
                        else:
                            desc, keep = self._desc(t, v, ins, part="text")
                            rid = sess.submit(desc=desc, prefix=made[key], credit_frames=credit0, **kw)
                            if credit0 is not None:
                                granted[rid] = credit0
                        index[rid] = i
                        continue
                    if prefix is not None:
                        self._check_prefix(prefix, v, ins)
                    desc, keep = self._desc(t, v, ins, part="whole" if prefix is None else "text")
                    rid = sess.submit(desc=desc, prefix=prefix, credit_frames=credit0, **kw)
                    index[rid] = i
                    if credit0 is not None:
                        granted[rid] = credit0

                def events():
                    if lead is None:
                        yield from sess.events()
                        return
                    while sess.open_ids:  # between events: each playing request's credit follows its playback clock
                        now, live = time.monotonic(), sess.open_ids
                        nxt = now + 4 * frame_s   # when the earliest next grant falls due
                        for r, t0 in started.items():
                            if r in live and r in granted:
                                want = int((now - t0 + lead) / frame_s) // 4 * 4
                                if want > granted[r]:
                                    sess.grant(r, want - granted[r])
                                    granted[r] = want
                                nxt = min(nxt, t0 + (granted[r] + 4) * frame_s - lead)
                        ev = sess.next(max(1, int((nxt - now) * 1000)))
                        if ev is not None:
                            yield ev

                for rid, kind, pcm, is_final, res in events():
                    if kind == _abi.EV_CHUNK:
                        started.setdefault(rid, time.monotonic())
                        yield index[rid], pcm, is_final
                    elif kind == _abi.EV_PREFIX and res.status == 0:
                        continue
                    elif kind != _abi.EV_DONE:
                        raise _abi.Q3Error(f"generation failed with status {res.status if res is not None else kind}")
            finally:
                for x in made.values():
                    x.close()

    def stream_text_with_voice(self, pieces, voice: VoiceFile, instruct=None, *, prefix=None, seed=None):
        """Speech for text that is still being written (an extension; include/q3tts.h, "streaming text input"). pieces: an iterator of
        strings or id lists, e.g. the words a language model emits; the first non-empty piece starts the request, the others are fed
        from a helper thread as the iterator yields them, and its end closes the text. Yields (f32 chunk, is_final) as the 4-frame
        chunks are produced: the first can sound once 5 text ids exist, long before the sentence is complete.

        Each piece is tokenised on its own, so cut at word boundaries (keep the leading space with the next word, as the tokenizer's
        pre-tokeniser would): a piece that ends inside a word gives other ids than the whole text. The audio is that of the streamed
        layout for the concatenated ids, however they were cut and whenever they arrived; it is NOT the audio of generate_with_voice
        for the same text (another prompt layout)."""
        import threading
        sc = self.sampler_config
        if prefix is not None:
            self._check_prefix(prefix, voice, instruct)
        it = iter(pieces)
        first = np.zeros(0, dtype=np.uint32)
        ended = False
        while first.size == 0:
            try:
                first = self._encode(next(it))
            except StopIteration:
                ended = True
                break
        if first.size == 0:
            raise ValueError("stream_text_with_voice: the pieces hold no text")
        desc, keep = self._desc(first, voice, instruct, part="whole" if prefix is None else "text")
        with native.NativeSession(self._native) as sess:
            rid = sess.submit(desc=desc, temperature=sc.temperature, top_k=sc.top_k, top_p=sc.top_p, seed=sc.seed if seed is None else seed,
                              max_steps=self.max_steps, prefix=prefix, text_stream=True, text_open=not ended)
            failure = []
            gate, live = threading.Lock(), [True]  # the feeder touches the session only while the consumer is inside this block

            def feed():
                try:
                    for piece in it:
                        ids = self._encode(piece)
                        with gate:
                            if not live[0]:
                                return
                            if ids.size:
                                sess.append_text(rid, ids)
                    with gate:
                        if live[0]:
                            sess.append_text(rid, None, close=True)
                except Exception as ex:  # the request ended meanwhile (EOS, max_steps), or the iterator failed
                    failure.append(ex)
                    with gate:
                        if live[0]:
                            try:
                                sess.cancel(rid)
                            except _abi.Q3Error:
                                pass
            th = threading.Thread(target=feed, daemon=True) if not ended else None
            if th is not None:
                th.start()
            try:
                for _, kind, pcm, is_final, res in sess.events():
                    if kind == _abi.EV_CHUNK:
                        yield pcm, is_final
                    elif kind == _abi.EV_CANCELLED and failure:
                        raise failure[0]
                    elif kind != _abi.EV_DONE:
                        raise _abi.Q3Error(f"generation failed with status {res.status if res is not None else kind}")
            finally:
                with gate:   # (also when the consumer stops early: the feeder ends at its next piece, the session closes below)
                    live[0] = False

    def load_clone_encoders(self, clone_config=None):
        """The reference loads onnx/qwen3_tts_codec_encoder.onnx and onnx/qwen3_tts_speaker_encoder.onnx when they exist
        (src/tts/engine.rs:105-119). Those graphs are not available; this loads the family-structure encoders with seeded
        synthetic weights (q3tts_clone_init)."""
        if clone_config is None:
            clone_config = _abi.CloneConfig()
            self._native.lib.q3tts_clone_default_config(clone_config)
            clone_config.se_dim = self.cfg.model.d_embed
            clone_config.ae_n_codebooks = self.cfg.model.n_codebooks
            clone_config.ae_codebook_size = self.cfg.model.codebook_size
        self._native.clone_init(clone_config)

    def _read_wav_any(self, path, resample=False):
        """create_voice_file's own WAV decoding (src/tts/engine.rs:339-373): f32 / i16 / i32, first channel, 24 kHz only. resample = True
        (an extension): a file at another rate is accepted, and its first channel converted to 24 kHz by the device resampler."""
        with open(path, "rb") as f:
            raw = f.read()
        if raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
            raise _abi.Q3Error("WAV error: not a RIFF/WAVE file")
        pos, fmt, data = 12, None, None
        while pos + 8 <= len(raw):
            cid, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
            body = raw[pos + 8:pos + 8 + size]
            if cid == b"fmt ":
                fmt = struct.unpack("<HHIIHH", body[:16])
                if fmt[0] == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: sub-format tag
                    fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
            elif cid == b"data":
                data = body
            pos += 8 + size + (size & 1)
        if fmt is None or data is None:
            raise _abi.Q3Error("WAV error: missing fmt or data chunk")
        tag, channels, rate, _, _, bits = fmt
        if rate != 24000 and not resample:
            raise _abi.Q3Error(f"Expected 24000Hz audio, found {rate}Hz")
        if tag == 3 and bits == 32:
            a = np.frombuffer(data[:len(data) // 4 * 4], dtype="<f4").astype(np.float32)
        elif tag == 1 and bits == 16:
            a = np.frombuffer(data[:len(data) // 2 * 2], dtype="<i2").astype(np.float32) / np.float32(32768.0)
        elif tag == 1 and bits == 32:
            a = (np.frombuffer(data[:len(data) // 4 * 4], dtype="<i4").astype(np.float32) / np.float32(2147483648.0)).astype(np.float32)
        else:
            raise _abi.Q3Error(f"Unsupported WAV format: {'Float' if tag == 3 else 'Int'} {bits} bits")
        a = a[::channels].copy() if channels > 1 else a
        return a if rate == 24000 else self._native.resample(a, rate, 24000)

    def create_voice_file(self, audio_path, ref_text, *, resample=False):  # src/tts/engine.rs:324-387
        """resample = True: a clip at 8, 16, 44.1, 48 kHz, ... is converted to 24 kHz first (q3tts_resample); the default refuses it with
        the reference's error."""
        if not hasattr(self._native, "clone_cfg"):
            raise _abi.Q3Error("AudioEncoder not loaded. Please ensure models/onnx/qwen3_tts_codec_encoder.onnx exists.")
        audio = self._read_wav_any(audio_path, resample)
        codes = self._native.audio_encode(audio)            # "Extracting audio codes..."
        emb = self._native.speaker_encode(audio)            # "Extracting speaker embedding..."
        return VoiceFile.new(ref_text, codes.reshape(-1).tolist(), emb.tolist())

    def _process_reference(self, audio_path, *, resample=False):  # src/tts/engine.rs:275-302 (TTSC cache beside the audio file)
        """resample = True: a file whose rate is not 24000 Hz is converted, channel by channel, before it reaches the encoders (the
        default hands the samples over whatever the file's rate says, as the reference does)."""
        cache_path = os.path.splitext(str(audio_path))[0] + ".cache"
        if os.path.exists(cache_path):
            try:
                return load_cache(cache_path)
            except (ValueError, struct.error, OSError):
                pass
        audio = AudioSample.load_wav(audio_path)
        if not hasattr(self._native, "clone_cfg"):
            raise _abi.Q3Error("AudioEncoder not loaded (required for processing raw audio)")
        samples = audio.samples
        if resample and audio.sample_rate != 24000:
            ch = max(1, audio.channels)
            samples = np.stack([self._native.resample(samples[c::ch], audio.sample_rate, 24000) for c in range(ch)], axis=1).reshape(-1)
        codes = self._native.audio_encode(samples).reshape(-1).tolist()
        emb = self._native.speaker_encode(samples).tolist()
        try:
            save_cache(cache_path, codes, emb)
        except OSError:
            pass
        return codes, emb

    def generate(self, text, ref_audio_path, ref_text, instruct=None, *, resample=False):  # src/tts/engine.rs:243-272
        codes, emb = self._process_reference(ref_audio_path, resample=resample)
        return self.generate_with_voice(text, VoiceFile.new(ref_text, codes, emb), instruct)


def cleanup():
    """qwen3_tts::cleanup() (src/lib.rs:18-20): llama_backend_free in the reference; nothing global to free here."""
    return None
