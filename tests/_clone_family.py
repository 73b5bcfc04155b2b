"""The model family's own modules loaded with the clone oracle's seeded weights (tests/test_clone_family_cpu.py, tests/test_clone_shapes_cpu.py).

ECAPA_TimeDelayNet (qwen2_5_omni) for the speaker encoder and MimiModel's encoder / encoder_transformer / downsample / quantizer for the audio
encoder, as the installed transformers package holds them, for any q3tts clone config the modules can express. CPU only; structure only.
"""
import numpy as np
import torch

import _oracle as O


def _tid(comp, w):
    return (5 << 16) | (comp << 8) | w


def _conv_w(comp, ww, cin, n, k, bias):
    kp = (k * cin + 511) // 512 * 512
    std = np.float32(1.0) / np.sqrt(np.float32(k * cin))
    W = O.synth_tensor(0, _tid(comp, ww), (n, kp), 0.0, float(std), True)[:, :k * cin].reshape(n, k, cin).transpose(0, 2, 1)
    b = O.synth_tensor(0, _tid(comp, ww + 1), (n,), 0.0, 0.02, False) if bias else None
    return torch.from_numpy(np.ascontiguousarray(W)), (None if b is None else torch.from_numpy(b))


def _put(conv, comp, ww, cin, n, k, bias=True):
    W, b = _conv_w(comp, ww, cin, n, k, bias)
    assert conv.weight.shape == W.shape, (conv.weight.shape, W.shape)
    conv.weight.data.copy_(W)
    if bias:
        conv.bias.data.copy_(b)


def _vec(comp, w, n, base, std):
    return torch.from_numpy(O.synth_tensor(0, _tid(comp, w), (n,), base, std, False))


def speaker_reflect_pad(c):
    """the widest reflect padding of the speaker encoder: torch's reflect mode needs more frames than this"""
    return max(c.se_dilations[i] * (c.se_kernels[i] - 1) // 2 for i in range(5))


def ecapa(c):
    """ECAPA_TimeDelayNet of clone config c with the oracle's weights of seed 0 (f32, eval)"""
    from transformers.models.qwen2_5_omni.configuration_qwen2_5_omni import Qwen2_5OmniDiTConfig
    from transformers.models.qwen2_5_omni.modeling_qwen2_5_omni import ECAPA_TimeDelayNet
    cfg = Qwen2_5OmniDiTConfig(mel_dim=128, enc_channels=list(c.se_channels), enc_kernel_sizes=list(c.se_kernels), enc_dilations=list(c.se_dilations),
       enc_attention_channels=c.se_attn_channels, enc_res2net_scale=c.se_res2net_scale, enc_se_channels=c.se_se_channels, enc_dim=c.se_dim)
    m = ECAPA_TimeDelayNet(cfg).eval()
    C, C4, S = c.se_channels[0], c.se_channels[4], c.se_res2net_scale
    _put(m.blocks[0].conv, 0, 0, 128, C, c.se_kernels[0])
    for i in (1, 2, 3):
        b = m.blocks[i]
        _put(b.tdnn1.conv, i, 0, C, C, 1); _put(b.tdnn2.conv, i, 2, C, C, 1)
        _put(b.se_block.conv1, i, 4, C, c.se_se_channels, 1); _put(b.se_block.conv2, i, 6, c.se_se_channels, C, 1)
        for p in range(1, S): _put(b.res2net_block.blocks[p - 1].conv, i, 16 + 2 * p, C // S, C // S, c.se_kernels[i])
    _put(m.mfa.conv, 8, 0, 3 * C, C4, c.se_kernels[4]); _put(m.asp.tdnn.conv, 9, 0, 3 * C4, c.se_attn_channels, 1)
    _put(m.asp.conv, 10, 0, c.se_attn_channels, C4, 1); _put(m.fc, 11, 0, 2 * C4, c.se_dim, 1)
    return m


def ecapa_run(m, mel):
    """[T][128] -> [se_dim], in the module's own dtype"""
    p = next(m.parameters())
    with torch.no_grad():
        return m(torch.from_numpy(mel).to(p.dtype)[None]).numpy()[0]


def mimi(c, max_rows=8000):
    """MimiModel of clone config c (ae_down_stride must be 2, at least two codebooks, a power-of-two codebook) with the oracle's weights"""
    from transformers.models.mimi.configuration_mimi import MimiConfig
    from transformers.models.mimi.modeling_mimi import MimiModel
    ratios = list(c.ae_ratios)[:c.ae_n_ratios]
    enc_rate = -(-24000 // int(np.prod(ratios)))
    cfg = MimiConfig(sampling_rate=24000, audio_channels=1, hidden_size=c.ae_hidden, num_filters=c.ae_filters, num_residual_layers=1,
       upsampling_ratios=ratios[::-1], kernel_size=c.ae_kernel, last_kernel_size=c.ae_last_kernel, residual_kernel_size=c.ae_res_kernel,
       dilation_growth_rate=2, use_causal_conv=True, pad_mode="constant", compress=2, codebook_size=c.ae_codebook_size, codebook_dim=c.ae_vq_dim,
       num_quantizers=c.ae_n_codebooks, num_semantic_quantizers=1, use_conv_shortcut=False, vector_quantization_hidden_dimension=c.ae_vq_dim,
       upsample_groups=c.ae_hidden, num_hidden_layers=c.ae_n_layer, intermediate_size=c.ae_d_ffn, num_attention_heads=c.ae_n_head,
       num_key_value_heads=c.ae_n_head, head_dim=c.ae_head_dim, hidden_act="gelu_pytorch_tanh", max_position_embeddings=max(8000, max_rows), norm_eps=c.ae_ln_eps,
       rope_theta=c.ae_rope_theta, sliding_window=c.ae_window, layer_scale_initial_scale=c.ae_layer_scale, frame_rate=enc_rate / 2, attn_implementation="eager")
    m = MimiModel(cfg).eval()
    C = c.ae_filters
    L = m.encoder.layers
    _put(L[0].conv, 32, 0, 1, C, c.ae_kernel)
    li = 1
    for i in range(c.ae_n_ratios):
        r = c.ae_ratios[i]; comp = 33 + 4 * i
        _put(L[li].block[1].conv, comp, 0, C, C // 2, c.ae_res_kernel); _put(L[li].block[3].conv, comp + 1, 0, C // 2, C, 1)
        _put(L[li + 2].conv, comp + 2, 0, C, 2 * C, 2 * r)
        li += 3; C *= 2
    _put(L[li + 1].conv, 60, 0, C, c.ae_hidden, c.ae_last_kernel)
    H, dq = c.ae_hidden, c.ae_n_head * c.ae_head_dim
    for l, lay in enumerate(m.encoder_transformer.layers):
        comp = 64 + l
        lay.input_layernorm.weight.data.copy_(_vec(comp, 0, H, 1.0, 0.05)); lay.input_layernorm.bias.data.copy_(_vec(comp, 1, H, 0.0, 0.02))
        lay.post_attention_layernorm.weight.data.copy_(_vec(comp, 5, H, 1.0, 0.05)); lay.post_attention_layernorm.bias.data.copy_(_vec(comp, 6, H, 0.0, 0.02))
        ls = np.float32(c.ae_layer_scale)
        lay.self_attn_layer_scale.scale.data.copy_(_vec(comp, 4, H, float(ls), float(np.float32(0.1) * ls)))
        lay.mlp_layer_scale.scale.data.copy_(_vec(comp, 9, H, float(ls), float(np.float32(0.1) * ls)))
        Wqkv, _ = _conv_w(comp, 2, H, 3 * dq, 1, False); Wqkv = Wqkv[:, :, 0]
        lay.self_attn.q_proj.weight.data.copy_(Wqkv[:dq]); lay.self_attn.k_proj.weight.data.copy_(Wqkv[dq:2 * dq]); lay.self_attn.v_proj.weight.data.copy_(Wqkv[2 * dq:])
        lay.self_attn.o_proj.weight.data.copy_(_conv_w(comp, 3, dq, H, 1, False)[0][:, :, 0])
        lay.mlp.fc1.weight.data.copy_(_conv_w(comp, 7, H, c.ae_d_ffn, 1, False)[0][:, :, 0])
        lay.mlp.fc2.weight.data.copy_(_conv_w(comp, 8, c.ae_d_ffn, H, 1, False)[0][:, :, 0])
    _put(m.downsample.conv, 100, 0, H, H, 2 * c.ae_down_stride, bias=False)
    q = m.quantizer
    _put(q.semantic_residual_vector_quantizer.input_proj, 101, 0, H, c.ae_vq_dim, 1, bias=False)
    _put(q.acoustic_residual_vector_quantizer.input_proj, 102, 0, H, c.ae_vq_dim, 1, bias=False)
    D = c.ae_vq_dim
    cbstd = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    books = [O.synth_tensor(0, _tid(110 + k, 0), (c.ae_codebook_size, D), 0.0, cbstd, False) for k in range(c.ae_n_codebooks)]
    q.semantic_residual_vector_quantizer.layers[0].codebook.embed_sum.data.copy_(torch.from_numpy(books[0]))
    for k in range(1, c.ae_n_codebooks): q.acoustic_residual_vector_quantizer.layers[k - 1].codebook.embed_sum.data.copy_(torch.from_numpy(books[k]))
    return m


def mimi_run(m, a):
    """24 kHz clip -> (pre-quantiser rows [frames][hidden], ids [frames][n_codebooks]), in the module's own dtype"""
    p = next(m.parameters())
    with torch.no_grad():
        emb = m.encoder(torch.from_numpy(a).to(p.dtype)[None, None])
        h = m.encoder_transformer(emb.transpose(1, 2))[0].transpose(1, 2)
        lat = m.downsample(h)
        codes = m.quantizer.encode(lat).transpose(0, 1)[0].T.numpy()
    return lat[0].T.numpy(), codes


def to_float64(m):
    """a float64 copy of a loaded module (weights, codebook buffers and all)"""
    import copy
    return copy.deepcopy(m).double()
