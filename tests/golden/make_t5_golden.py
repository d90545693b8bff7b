"""Writes tests/golden/t5_encoder.npz: what ``transformers.T5EncoderModel`` (eval mode, float32, CPU) computes for the cases of
tests/t5_common.py, with weights from ``init_fill.fill`` under the state_dict key names.  Only the schema, the inputs and the outputs are
stored; no weights.  Needs ``transformers`` (run where it is installed: ``python tests/golden/make_t5_golden.py``); the tests need
neither it nor this script.

Also stored: the integer bucket of every relative distance -159 .. 159 from ``T5Attention._relative_position_bucket`` (distances 16, 32 and
64 sit exactly on boundaries of the logarithm, where the order of the float32 operations decides the bucket).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import t5_common as TC  # noqa: E402


def main():
    from transformers import T5Config, T5EncoderModel
    from transformers.models.t5.modeling_t5 import T5Attention
    out = {}
    for case in TC.CASES:
        spec = TC.CASE_SPECS[case]
        g = spec["geo"]
        cfg = T5Config(vocab_size=g["vocab"], d_model=g["d_model"], d_kv=g["d_kv"], d_ff=g["d_ff"], num_layers=g["layers"], num_heads=g["heads"],
                       relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0, layer_norm_epsilon=1e-6,
                       feed_forward_proj="gated-gelu" if g["gated"] else "relu")
        model = T5EncoderModel(cfg).eval()
        schema = TC.schema_of(**g)
        sd = TC.state_dict(schema)
        want = {k: tuple(v.shape) for k, v in model.state_dict().items() if k != "encoder.embed_tokens.weight"}
        assert want == {k: tuple(s) for k, s in schema}, "schema_of does not match T5EncoderModel.state_dict()"
        full = dict(sd)
        if "encoder.embed_tokens.weight" in model.state_dict():
            full["encoder.embed_tokens.weight"] = sd["shared.weight"]
        model.load_state_dict(full, strict=True)
        assert model.config.dense_act_fn == ("gelu_new" if g["gated"] else "relu")
        ids, mask = TC.case_inputs(case)
        with torch.no_grad():
            y = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask).to(torch.bool))["last_hidden_state"]
        out[f"{case}.schema"] = np.array(json.dumps([[k, list(s)] for k, s in schema]))
        out[f"{case}.input_ids"] = ids
        out[f"{case}.attention_mask"] = mask
        out[f"{case}.step"] = np.int64(spec["step"])
        out[f"{case}.out"] = y.numpy()[:, :, ::spec["step"]].astype(np.float32)
        print(case, tuple(y.shape), "max |y| =", float(y.abs().max()))
    rel = torch.arange(-159, 160, dtype=torch.long)
    out["bucket_row"] = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128).numpy().astype(np.int64)
    path = os.path.join(HERE, "t5_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
