"""The decoder with a sampling Predictor and a code-0 repetition penalty on the CPU — test infrastructure.

The frame loop of tests/_pred_q8.py::generate (itself pinned to q3o_generate) restated with the two controls of include/q3tts.h,
"Predictor sampler and repetition penalty", over the same exported primitives: the layers / head of _pred_q8, q3o_sample for every
code, q3o_rng_f32 for both draw streams. tests/test_pred_sample_cpu.py pins it: with the controls off it equals q3o_generate id for id.
"""
import numpy as np

import _oracle as O
from _pred_q8 import head, layers, mats_from_model  # noqa: F401  (mats_from_model: re-exported for the tests)

PRED_SEED_XOR = 0x9E3779B97F4A7C15


def apply_penalty(logits, seen, limit, p):
    """lg[i] = lg[i] > 0 ? lg[i] / p : lg[i] * p for every seen i < limit, in f32 (IEEE division), in place."""
    p = np.float32(p)
    idx = np.array(sorted(i for i in seen if i < limit), dtype=np.int64)
    if idx.size:
        v = logits[idx]
        with np.errstate(invalid="ignore"):
            logits[idx] = np.where(v > 0, (v / p).astype(np.float32), (v * p).astype(np.float32))


def generate(om, pred, prompt, temperature=0.0, top_k=40, top_p=0.9, seed=0, max_steps=16, min_frames=0, force_eos_at=-1,
             pred_sampler=(0.0, 0, 1.0), penalty=1.0, trace=None):
    """_pred_q8.generate with pred_sampler = (temperature, top_k, top_p) of the Predictor and the repetition penalty.
    Predictor draws: q3o_rng_f32(seed ^ PRED_SEED_XOR), draw frame * (ncb - 1) + (q - 1) serves code q. trace (a list): receives per
    Predictor code (frame, q, code, argmax of its own logits). Returns (codes [n_frames][n_codebooks], hit_eos)."""
    c, L = om.cfg, O.lib()
    dp, de, ncb, cbs = c.p_d_model, c.d_embed, c.n_codebooks, c.codebook_size
    pt, pk, pp = pred_sampler
    rows = [np.ascontiguousarray(prompt, dtype=np.float32)]
    draws = np.zeros(max(max_steps, 1), dtype=np.float32)
    L.q3o_rng_f32(seed, draws.size, O.ptr(draws, O.f32p))
    pdraws = np.zeros(max(max_steps, 1) * (ncb - 1), dtype=np.float32)
    L.q3o_rng_f32(seed ^ PRED_SEED_XOR, pdraws.size, O.ptr(pdraws, O.f32p))
    n_draw = 0
    pad = np.zeros(de, dtype=np.float32)
    if c.tts_pad_id < c.text_vocab:
        L.q3o_text_embedding(om.h, c.tts_pad_id, O.ptr(pad, O.f32p))

    def codec(q, code):
        e = np.zeros(de, dtype=np.float32)
        L.q3o_codec_embedding(om.h, q, int(code), O.ptr(e, O.f32p))
        return e

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
                apply_penalty(logits, seen, c.sample_limit, penalty)
            r = 0.0
            if temperature > 0.0:
                r = float(draws[n_draw]); n_draw += 1
            code0 = L.q3o_sample(O.ptr(logits, O.f32p), c.sample_limit, temperature, top_k, top_p, r)
            seen.add(int(code0))
        if code0 == c.eos_code:
            hit_eos = True
            break
        frame = [code0]
        emb = codec(0, code0)
        pin = np.stack([project(hid), project(emb)])
        fb = (np.float32(0.0) + emb).astype(np.float32)
        cache = [[] for _ in range(pred.L)]
        px = layers(pred, pin, 0, cache=cache)
        pl = head(pred, px[1], 0, cbs)
        for q in range(1, ncb):
            pl = np.ascontiguousarray(pl, dtype=np.float32)
            r = float(pdraws[step * (ncb - 1) + (q - 1)]) if pt > 0.0 else 0.0
            mi = int(L.q3o_sample(O.ptr(pl, O.f32p), cbs, pt, pk, pp, r))
            if trace is not None:
                trace.append((step, q, mi, int(np.argmax(pl))))
            frame.append(mi)
            emb = codec(q, mi)
            fb = (fb + emb).astype(np.float32)
            if q < ncb - 1:
                px = layers(pred, project(emb)[None, :], q + 1, cache=cache)
                pl = head(pred, px[0], q * cbs, cbs)
        codes.append(frame)
        fb = (fb + pad).astype(np.float32)
        rows.append(fb[None, :])
        hid, logits = om.talker_prefill(np.concatenate(rows))
    return np.array(codes, dtype=np.int32).reshape(-1, ncb), hit_eos


# ---- the inputs of tests/test_pred_sample_gpu.py (test_pred_sample_cpu.py asserts that a greedy Predictor / no penalty would fail them) ----
N_CTX = 256
FRAMES = 8
PROMPT_IDS = np.arange(100, 120)
# (a greedy Talker carries a seed too: the Predictor's draws derive from the request's seed, and a request without one takes the wall clock)
TALKERS = {"greedy": dict(temperature=0.0, seed=3), "sampled": dict(temperature=0.7, top_k=40, top_p=0.9, seed=11)}
# (temperature, top_k, top_p): the select path (top_k < limit) | the full bitonic sort + the top-p cut | top_k = 1: must equal greedy
PRED_CONFIGS = {"select": (0.9, 50, 1.0), "sort_top_p": (1.0, 0, 0.8), "top1": (0.7, 1, 1.0)}
PENALTY = 1.3


def spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def prompt(om, ids=PROMPT_IDS):
    desc, keep = O.make_prompt_desc(np.asarray(ids), spk_emb=spk(om.cfg.d_embed))
    return om.build_prompt(desc)


def request(talker, frames=FRAMES):
    return dict(TALKERS[talker], max_steps=frames, min_frames=frames)


# penalty cases: inputs whose unpenalised code-0 sequence repeats a code within FRAMES frames (so that the penalty has something to change)
PENALTY_CASES = {"greedy": (np.arange(120, 140), dict(temperature=0.0, seed=3)),
                 "sampled": (PROMPT_IDS, dict(temperature=0.7, top_k=40, top_p=0.9, seed=13))}


def tiny_cfg(max_batch=4, with_vocoder=0, pred_q8=0, wide=False):
    """_abi.tiny_config; wide: codebook_size = codecq_rows = 2048 (NP = 2048 and 16 candidates per thread in the sampler's select path)."""
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=N_CTX, with_vocoder=with_vocoder)
    cfg.predictor_q8_0 = pred_q8
    if wide:
        cfg.model.codebook_size = cfg.model.codecq_rows = 2048
    return cfg


def batch_requests(om):
    """Seven requests of mixed lengths and distinct seeds for 4 slots (three slots are refilled), Talker sampled."""
    rng = np.random.default_rng(7)
    reqs = []
    for i in range(7):
        pe = prompt(om, rng.integers(0, 151643, size=int(rng.integers(3, 30))))
        t = [3, 9, 5, 12, 7, 4, 10][i]
        reqs.append(dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=70 + i, max_steps=16, min_frames=t, force_eos_at=t))
    return reqs


def differing(trace):
    """(Predictor codes that are not the argmax of their own logits, Predictor codes)."""
    return sum(1 for t in trace if t[2] != t[3]), len(trace)
