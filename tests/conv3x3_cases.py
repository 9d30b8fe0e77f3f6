"""
The shapes of the isolated gance::conv3x3 checks, shared by tests/test_conv3x3.py (which ties them to the dispatcher: every
kernel form that VGG16 reaches at a judged side up to 256 must have a case here) and tests/test_conv3x3_gpu.py (which runs them).
"""

# (batch, cin, cout, side): the smallest shapes at which each thing can go wrong
CASES = (
    (1, 16, 16, 4),  # smaller than any tile, one chunk, one channel tile
    (3, 16, 48, 5),  # odd side, the 32-channel block with its second channel tile cut
    (1, 48, 16, 10),  # an odd number of chunks
    (3, 48, 80, 33),  # channel tile and pixel tile both cut
    (1, 16, 64, 34),  # conv1_1's shape class
    (1, 64, 64, 64),
    (1, 16, 16, 130),  # partial tiles on both axes past a multiple of every tile side
    (1, 512, 512, 4),  # longest K, sixteen splits
    (1, 512, 512, 16),  # longest K, sixteen splits
    (3, 256, 512, 8),  # eight splits
    (1, 128, 256, 32),  # four splits
    # one case on each side of every boundary the form has in the side, at the smallest channel counts that take the form
    (1, 64, 16, 64),  # two splits up to side 64 ...
    (1, 64, 16, 65),  # ... none above
    (1, 128, 16, 32),  # four splits up to side 32 ...
    (1, 128, 16, 33),  # ... two above
    (1, 512, 16, 16),  # sixteen splits up to side 16 ...
    (1, 512, 16, 17),  # ... four above
    (1, 16, 64, 65),  # the 64-channel block without a split, with cut tiles
)

# (cin, cout) of VGG16's thirteen convolutions (conv1_1 with its input padded to 16 channels)
VGG_LAYERS = (
    (16, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256),
    (256, 512), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512),
)  # fmt: skip
