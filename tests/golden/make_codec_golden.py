"""Writes tests/golden/codec_segments.npz: what ``transformers.EncodecModel(...).decode(codes, scales)`` (eval mode, float32, CPU) returns
for three overlapping chunks of 12 frames (chunk_length_s = 0.08 at 48 kHz: chunk 3840, stride 3801), B = 2, with weights from
``init_fill.fill`` under the key schema tests/golden/encodec.npz carries and codes / scales from ``init_fill`` too
(tests/codec_segments_common.py golden_codes_and_scales).  Only the output is stored.  Needs ``transformers`` (run where it is installed:
``python tests/golden/make_codec_golden.py``); the tests need neither it nor this script.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import codec_segments_common as CC  # noqa: E402


def main():
    from transformers import EncodecConfig, EncodecModel
    cfg = EncodecConfig(sampling_rate=48000, audio_channels=2, normalize=True, chunk_length_s=CC.GOLDEN_SEGMENT_S, overlap=CC.GOLDEN_OVERLAP,
                        use_causal_conv=False, norm_type="time_group_norm")
    model = EncodecModel(cfg).eval()
    assert (cfg.chunk_length, cfg.chunk_stride) == (CC.GOLDEN_CHUNK, CC.GOLDEN_STRIDE), (cfg.chunk_length, cfg.chunk_stride)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))        # noqa: E731
    p = CC.dec_params()
    assert {k: tuple(v.shape) for k, v in model.decoder.state_dict().items()} == {k: v.shape for k, v in p.items()}
    model.decoder.load_state_dict({k: T(v) for k, v in p.items()}, strict=True)
    tables = CC.tables(CC.GOLDEN_NQ)
    assert len(model.quantizer.layers) == CC.GOLDEN_NQ
    with torch.no_grad():
        for i, layer in enumerate(model.quantizer.layers):
            layer.codebook.embed.copy_(T(tables[i]))
        codes, scales = CC.golden_codes_and_scales()
        y = model.decode(T(codes), [T(s) for s in scales])[0]
    want = (CC.GOLDEN_B, 2, CC.GOLDEN_STRIDE * (len(CC.GOLDEN_COUNTS) - 1) + CC.GOLDEN_CHUNK)
    assert tuple(y.shape) == want == (2, 2, 11442), y.shape
    path = os.path.join(HERE, "codec_segments.npz")
    np.savez_compressed(path, **{"decode.y": y.numpy().astype(np.float32)})
    print("wrote", path, os.path.getsize(path), "bytes; max |y| =", float(y.abs().max()))


if __name__ == "__main__":
    main()
