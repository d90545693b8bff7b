"""``engine.conv_traffic``: the algorithmic traffic / work of a convolution (weights once + conv input + output),
which bench.py sums into the roofline figures.  One case per way a layer can run; the expected numbers are written out by hand from the
formula each form used when it kept its own copy:

    launch      w = (taps c + cx) M es                act = B Lin (c + cx) es + B Ly out_C (4 if y_f32 else es)
    deep phase  w = (taps c + cx) M (1 if fp8 else es) + (4 M if fp8)        act = ... + B Ly out_C es
    tile phase  as the launch
    long phase  as the launch, never y_f32
    flops = 2 (taps c + cx) M B Lout in all four

c: unpadded channels of the conv sources, cx: of the extra K segments, es: bytes of the compute dtype.
"""
import pytest

from jen1_amd.engine import conv_traffic

CASES = {
    # the FiLM GEMM of the time tables: bf16 operands, float32 output
    "launch bf16, y_f32": (dict(taps=1, c_real=512, c_extra=0, M=768, B=1, L_in=4, L_out=4, L_y=4, out_C=768, w_es=2, act_es=2, out_es=4),
                           (512 * 768 * 2, 4 * 512 * 2 + 4 * 768 * 4, 2 * 512 * 768 * 4)),
    # a sub-pixel upsampling launch: M = out_C * factor, more output rows than GEMM columns
    "launch bf16, sub-pixel": (dict(taps=2, c_real=256, c_extra=0, M=512, B=2, L_in=94, L_out=95, L_y=375, out_C=128, w_es=2, act_es=2, out_es=2),
                               (524288, 96256 + 192000, 99614720)),
    # JEN1_FP8: 1-byte weights + one float32 scale per output row; activations stay bf16
    "deep phase fp8, two sources": (dict(taps=3, c_real=256 + 256, c_extra=0, M=512, B=2, L_in=24, L_out=24, L_y=24, out_C=512, w_es=1, act_es=2,
                                         out_es=2, scale_bytes=4 * 512),
                                    (786432 + 2048, 49152 + 49152, 75497472)),
    # a block's second conv with its 1x1 shortcut riding along as two extra K segments (float32)
    "tile phase f32, two extras": (dict(taps=3, c_real=128, c_extra=128 + 128, M=128, B=2, L_in=375, L_out=375, L_y=375, out_C=128, w_es=4,
                                        act_es=4, out_es=4),
                                   (327680, 1152000 + 384000, 122880000)),
    # an up-path block's first conv: the skip is the second source
    "long phase bf16, second source": (dict(taps=3, c_real=128 + 128, c_extra=0, M=128, B=4, L_in=1500, L_out=1500, L_y=1500, out_C=128, w_es=2,
                                            act_es=2, out_es=2),
                                       (196608, 3072000 + 1536000, 1179648000)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_conv_traffic(name):
    kw, want = CASES[name]
    got = conv_traffic(kw["taps"], kw["c_real"], kw["c_extra"], kw["M"], kw["B"], kw["L_in"], kw["L_out"], kw["L_y"], kw["out_C"],
                       **{k: v for k, v in kw.items() if k in ("w_es", "act_es", "out_es", "scale_bytes")})
    assert got == want and all(isinstance(v, int) for v in got), (name, got, want)
