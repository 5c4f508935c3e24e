"""The models tests/test_conv1_fc_host.py plans and tests/test_gpu_conv1_fc.py runs: a one-channel convolution -> Reshape ->
FullyConnected (-> Softmax), each the smallest shape at which one path of conv1_fc_rt (k_conv1_fc.hip) can go wrong.

    id: (H, W), stem = (kind, N, KH, KW, (sh, sw), padding), classes, u8, FullyConnected weight zero point offset, softmax, wmax
"""
CASES = {
    # K a multiple of 64; the stage sits over the fc_rowwave_softmax<4> group; three bands, the last of two rows
    "a": ((10, 8), ("dw", 8, 3, 3, (1, 1), "same"), 4, False, 0, True, None),
    # odd H: uneven SAME padding; K = 120: K % 16 != 0, the last k step masked for the weights and the ones row; byte-edge stores
    "b": ((9, 12), ("conv", 4, 4, 3, (2, 2), "same"), 3, True, 5, False, None),
    # unequal strides, VALID; 12 of a tile's 16 rows; a band edge inside a k step (k0 = 288); three launches without the group
    "c": ((12, 16), ("conv", 12, 5, 2, (1, 2), "valid"), 12, False, 0, True, None),
    # a filter larger than half the image; three FullyConnected row tiles, the last one partial
    "d": ((20, 12), ("dw", 8, 10, 8, (2, 2), "same"), 35, False, 0, True, None),
    # 25 bands; narrow weights: the saturating-pack epilogue; 125 KiB of FullyConnected image: read through the L2
    "e": ((49, 40), ("dw", 16, 10, 8, (2, 2), "same"), 12, False, 0, True, 24),
    # the motivating model: speech.tflite retrained to 12 keywords with a Conv2D stem
    "f": ((49, 40), ("conv", 8, 10, 8, (2, 2), "same"), 12, True, -7, True, None),
    # four pixels per tile (N = 4, KW + 3 <= 16), OW = 10 not a multiple of them; a band edge off every 16-byte k piece (k0 = 280)
    "g": ((12, 12), ("conv", 4, 3, 3, (1, 1), "valid"), 5, False, 3, True, None),
}


def out_hw(shape, stem):
    (H, W), (_, _, KH, KW, (sh, sw), padding) = shape, stem
    if padding == "same":
        return -(-H // sh), -(-W // sw)
    return (H - KH) // sh + 1, (W - KW) // sw + 1


def build(name, seed=0):
    """the .tflite bytes of case `name` (tools/tflite_writer.kws_like)"""
    import numpy as np

    import tflite_writer as tw

    shape, stem, classes, u8, fc_wzp, softmax, wmax = CASES[name]
    rng = np.random.default_rng(1000 + seed + ord(name))
    return tw.kws_like(rng, shape, stem, classes, elem=tw.UINT8 if u8 else tw.INT8, fc_wzp=fc_wzp, softmax=softmax, wmax=wmax)
