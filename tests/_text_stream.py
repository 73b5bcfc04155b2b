"""The streamed text layout on the CPU — test infrastructure (include/q3tts.h, "streaming text input").

The frame loop of tests/_pred_sample.py::generate restated over the same exported primitives, with the row that is added to the feedback sum
(its line 90: `fb + pad`) as a function of the step: text[T[step]] while step < len(T), tts_pad afterwards. With no trailing rows and today's
prompt it is that loop, and tests/test_text_stream_cpu.py pins it to q3o_generate id for id. The streamed prompt's text part (two rows
instead of n + 3) is built here from the oracle's own look-ups; parity with upstream is unpinned (the reference crate has only the whole-text
layout), so the layout as include/q3tts.h states it is the contract.
"""
import numpy as np

import _oracle as O
import _pred_sample as S
from _pred_q8 import head, layers, mats_from_model  # noqa: F401  (mats_from_model: re-exported for the tests)

TTS_BOS, TTS_EOS = 151672, 151673
CODEC_PAD, CODEC_BOS = 2148, 2149
N_CTX = 256


def text_row(om, tid):
    e = np.zeros(om.cfg.d_embed, dtype=np.float32)
    O.lib().q3o_text_embedding(om.h, int(tid), O.ptr(e, O.f32p))
    return e


def codec_row(om, q, code):
    e = np.zeros(om.cfg.d_embed, dtype=np.float32)
    O.lib().q3o_codec_embedding(om.h, q, int(code), O.ptr(e, O.f32p))
    return e


def trailing(ids, closed=True):
    """T of the layout: the ids behind the first one, then tts_eos once the text is closed."""
    return [int(i) for i in ids[1:]] + ([TTS_EOS] if closed else [])


def voice_rows(om, **voice):
    """The voice part: the whole prompt of an empty text without its 3 text-part rows (BOS, EOS, the activation row)."""
    desc, keep = O.make_prompt_desc(np.zeros(0, dtype=np.uint32), **voice)
    return om.build_prompt(desc)[:-3]


def text_part(om, ids):
    """The streamed text part: today's first text-part row (text[tts_bos] + codec0[PAD]), then text[x[0]] + codec0[BOS]."""
    desc, keep = O.make_prompt_desc(np.zeros(0, dtype=np.uint32), spk_emb=S.spk(om.cfg.d_embed))
    bos_row = om.build_prompt(desc)[-3]
    return np.stack([bos_row, (text_row(om, ids[0]) + codec_row(om, 0, CODEC_BOS)).astype(np.float32)])


def prompt(om, ids, **voice):
    """(rows, T) of a streamed request: voice part ++ streamed text part, and the closed text's trailing ids."""
    if not voice:
        voice = dict(spk_emb=S.spk(om.cfg.d_embed))
    return np.concatenate([voice_rows(om, **voice), text_part(om, ids)]), trailing(ids)


def whole_prompt(om, ids, **voice):
    if not voice:
        voice = dict(spk_emb=S.spk(om.cfg.d_embed))
    desc, keep = O.make_prompt_desc(np.asarray(ids, dtype=np.uint32), **voice)
    return om.build_prompt(desc)


def generate(om, pred, prompt_rows, T=(), temperature=0.0, top_k=40, top_p=0.9, seed=0, max_steps=16, min_frames=0, force_eos_at=-1,
             pred_sampler=(0.0, 0, 1.0), penalty=1.0):
    """_pred_sample.generate with the addend of its line 90 as a function of the step: text[T[step]] for step < len(T), else tts_pad;
    the f32 order is (fb + codec_15) + row. Returns (codes [n_frames][n_codebooks], hit_eos)."""
    c, L = om.cfg, O.lib()
    dp, de, ncb, cbs = c.p_d_model, c.d_embed, c.n_codebooks, c.codebook_size
    pt, pk, pp = pred_sampler
    rows = [np.ascontiguousarray(prompt_rows, dtype=np.float32)]
    draws = np.zeros(max(max_steps, 1), dtype=np.float32)
    L.q3o_rng_f32(seed, draws.size, O.ptr(draws, O.f32p))
    pdraws = np.zeros(max(max_steps, 1) * (ncb - 1), dtype=np.float32)
    L.q3o_rng_f32(seed ^ S.PRED_SEED_XOR, pdraws.size, O.ptr(pdraws, O.f32p))
    n_draw = 0
    pad = np.zeros(de, dtype=np.float32)
    if c.tts_pad_id < c.text_vocab:
        L.q3o_text_embedding(om.h, c.tts_pad_id, O.ptr(pad, O.f32p))

    def addend(step):
        return text_row(om, T[step]) if step < len(T) else pad

    def project(x):
        y = np.zeros(dp, dtype=np.float32)
        L.q3o_project(om.h, O.ptr(np.ascontiguousarray(x, dtype=np.float32), O.f32p), O.ptr(y, O.f32p))
        return y
    codes, hit_eos, seen = [], False, set()
    hid, logits = om.talker_prefill(np.concatenate(rows))
    for step in range(max_steps):
        if force_eos_at >= 0 and step == force_eos_at:
            code0 = c.eos_code
        else:
            if step < min_frames and c.eos_code < c.sample_limit:
                logits[c.eos_code] = -np.inf
            if penalty != 1.0:
                S.apply_penalty(logits, seen, c.sample_limit, penalty)
            r = 0.0
            if temperature > 0.0:
                r = float(draws[n_draw]); n_draw += 1
            code0 = L.q3o_sample(O.ptr(logits, O.f32p), c.sample_limit, temperature, top_k, top_p, r)
            seen.add(int(code0))
        if code0 == c.eos_code:
            hit_eos = True
            break
        frame = [code0]
        emb = codec_row(om, 0, code0)
        pin = np.stack([project(hid), project(emb)])
        fb = (np.float32(0.0) + emb).astype(np.float32)
        cache = [[] for _ in range(pred.L)]
        px = layers(pred, pin, 0, cache=cache)
        pl = head(pred, px[1], 0, cbs)
        for q in range(1, ncb):
            pl = np.ascontiguousarray(pl, dtype=np.float32)
            r = float(pdraws[step * (ncb - 1) + (q - 1)]) if pt > 0.0 else 0.0
            mi = int(L.q3o_sample(O.ptr(pl, O.f32p), cbs, pt, pk, pp, r))
            frame.append(mi)
            emb = codec_row(om, q, mi)
            fb = (fb + emb).astype(np.float32)
            if q < ncb - 1:
                px = layers(pred, project(emb)[None, :], q + 1, cache=cache)
                pl = head(pred, px[0], q * cbs, cbs)
        codes.append(frame)
        fb = (fb + addend(step)).astype(np.float32)
        rows.append(fb[None, :])
        hid, logits = om.talker_prefill(np.concatenate(rows))
    return np.array(codes, dtype=np.int32).reshape(-1, ncb), hit_eos


# ---- the inputs of tests/test_text_stream_gpu.py (test_text_stream_cpu.py asserts that the whole-text layout would fail each of them) ----
FRAMES = 8
TALKERS = {"greedy": dict(temperature=0.0, seed=3), "sampled": dict(temperature=0.7, top_k=40, top_p=0.9, seed=11)}
# n_text = 1: T is tts_eos alone | 6: exhausted inside the second chunk | 40: never exhausted in 8 frames | an id beyond the text table
TEXTS = {
    "n1": np.array([4021], dtype=np.uint32),
    "n6": np.arange(300, 306, dtype=np.uint32),
    "n40": np.arange(1000, 1040, dtype=np.uint32),
    "oob": np.array([510, 200000, 511, 3000000, 512, 513], dtype=np.uint32),
}
PRED_SAMPLER = (0.9, 50, 1.0)


def request(talker, frames=FRAMES):
    return dict(TALKERS[talker], max_steps=frames, min_frames=frames)


def stream_desc(ids, d_embed):
    """(desc, keepalive) of a streamed request's prompt: the whole desc; text_stream = 1 makes the engine put only ids[0] into the prompt."""
    return O.make_prompt_desc(np.asarray(ids, dtype=np.uint32), spk_emb=S.spk(d_embed))


def batch_requests():
    """Seven requests for 4 slots (three slots are refilled): streamed and whole-text mixed, mixed text lengths and frame counts.
    Returns dicts with ids, stream, and the sampler / length keywords."""
    rng = np.random.default_rng(17)
    reqs = []
    for i in range(7):
        ids = rng.integers(0, 151643, size=[1, 9, 3, 30, 6, 2, 14][i]).astype(np.uint32)
        t = [4, 6, 3, 7, 5, 2, 6][i]
        reqs.append(dict(ids=ids, stream=i not in (1, 4), kw=dict(temperature=0.7, top_k=40, top_p=0.9, seed=170 + i, max_steps=16,
                                                                   min_frames=t, force_eos_at=t)))
    return reqs


def tiny_cfg(max_batch=4, with_vocoder=0, talker_q8=0):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=N_CTX, with_vocoder=with_vocoder)
    cfg.talker_q8_0 = talker_q8
    return cfg
