"""Engines of more than 64 slots: what tests/test_slots_cpu.py and tests/test_slots_gpu.py share — the bucket rule
restated, the request lists, and one engine per max_batch for the whole module (creation with its graph capture is the slow part)."""
import numpy as np

N_CTX = 256
SLOT_COUNTS = (64, 65, 128, 200, 256)


def buckets_le64(nb):
    """The row buckets of an engine with nb <= 64 slots, as the engine computed them before it took more: 1, 2, 4, 8, then the multiples
    of 16 below nb, then nb."""
    out = []
    r = 1
    while r < nb and r < 16:
        out.append(r)
        r *= 2
    r = 16
    while r < nb:
        out.append(r)
        r += 16
    out.append(nb)
    return out


def spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def base_rows(oracle, om, seed=21):
    """Two prompts of >= 40 rows built by the oracle: the requests take their last 1..40 rows."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=40), spk_emb=spk(om.cfg.d_embed) * (1.0 - 0.5 * k))
        out.append(om.build_prompt(desc))
    assert all(p.shape[0] >= 40 for p in out)
    return out


LONGEST = 99   # the one request of 24 frames: the batch's last live row is its own


def mixed_requests(bases, n=260, max_frames=24, pcm_every=3, seed0=0):
    """n sampled requests: prompts of 1..40 rows, forced lengths 1..max_frames - 1 frames (request LONGEST alone runs max_frames, so it
    finishes as the last live row), seed i, want_pcm on every pcm_every-th."""
    rng = np.random.default_rng(260)
    reqs = []
    for i in range(n):
        rows = int(rng.integers(1, 41))
        t = max_frames if i == LONGEST else int(rng.integers(1, max_frames))
        reqs.append(dict(embd=bases[i % 2][-rows:], temperature=0.7, top_k=40, top_p=0.9, seed=seed0 + i, max_steps=max_frames + 4, min_frames=t,
                         force_eos_at=t, want_pcm=1 if i % pcm_every == 0 else 0))
    assert {r["embd"].shape[0] for r in reqs} >= {1, 40} and {r["force_eos_at"] for r in reqs} >= {1, max_frames}
    return reqs


def oracle_kw(r):
    return {k: v for k, v in r.items() if k not in ("embd", "want_pcm", "desc")}


class Engines:
    """One tiny engine per max_batch, made on first use and kept until close()."""

    def __init__(self, **cfg_kw):
        self.cfg_kw, self.engs = cfg_kw, {}

    def cfg(self, max_batch):
        from q3tts import _abi
        cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=self.cfg_kw.get("n_ctx", N_CTX), with_vocoder=self.cfg_kw.get("with_vocoder", 1))
        cfg.talker_q8_0 = self.cfg_kw.get("talker_q8_0", 0)
        cfg.predictor_q8_0 = self.cfg_kw.get("predictor_q8_0", 0)
        return cfg

    def get(self, max_batch):
        from q3tts import native
        if max_batch not in self.engs:
            self.engs[max_batch] = native.NativeEngine(self.cfg(max_batch))
        return self.engs[max_batch]

    def close(self):
        for e in self.engs.values():
            e.close()
        self.engs = {}
