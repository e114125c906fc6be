"""Seeded inputs of the annotation tests and of tests/golden/make_golden_annotation.py: painted images of a few thousand pixels with a
legend of colours, label maps with their colour dictionaries, and -- for the nearest-pixel cases -- the brute-force *ambiguous mask*:
the pixels whose equidistant nearest valid pixels carry more than one label, where the reference (scipy's k-d tree), the host
statement and the device's smallest-index rule may each give another of the tied labels."""
import numpy as np

#: legends: the reference's default colours and an 11-colour one with components 0 and 255 and two colours one L1 step apart
LEGENDS = {
    'default4': [(0, 0, 255), (255, 0, 0), (0, 255, 0), (255, 229, 0)],
    'wide11': [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 0, 0), (127, 140, 141), (127, 140, 142),
               (0, 212, 255), (142, 68, 173), (255, 229, 0)],
}

#: name: (height, width, legend, seed, share of pixels that keep their legend colour)
PAINTED = {
    'small_default4': (24, 31, 'default4', 3, 0.5),
    'mid_wide11': (37, 53, 'wide11', 5, 0.3),
    'sparse_default4': (48, 70, 'default4', 7, 0.05),
    'sparse_wide11': (40, 64, 'wide11', 11, 0.02),
}

#: the largest ambiguous share a nearest-pixel case may have to be compared against the reference
AMBIGUOUS_CAP = 0.25


def blobs(height, width, nb_labels, seed):
    """a label map of `nb_labels` Voronoi cells of random sites: compact painted areas as an annotator leaves them"""
    rng = np.random.RandomState(seed)
    sites = np.stack([rng.randint(0, height, 3 * nb_labels), rng.randint(0, width, 3 * nb_labels)], axis=1)
    yy, xx = np.mgrid[0:height, 0:width]
    d2 = (yy[:, :, None] - sites[None, None, :, 0]) ** 2 + (xx[:, :, None] - sites[None, None, :, 1]) ** 2
    return (np.argmin(d2, axis=2) % nb_labels).astype(np.int64)


def painted(name):
    """(image uint8 [H, W, 3], colours, label map int64 [H, W], kept bool [H, W]): the map painted with the legend; the pixels outside
    `kept` carry noise that is none of the legend's colours"""
    height, width, legend, seed, keep = PAINTED[name]
    colors = LEGENDS[legend]
    segm = blobs(height, width, len(colors), seed)
    rng = np.random.RandomState(seed + 1000)
    kept = rng.rand(height, width) < keep
    kept[rng.randint(height), rng.randint(width)] = True
    image = np.array(colors, dtype=np.uint8)[segm]
    noise = rng.randint(0, 256, (height, width, 3)).astype(np.uint8)
    noise[:, :, 1] = np.where((noise[:, :, None, :] == np.array(colors, dtype=np.uint8)[None, None]).all(axis=3).any(axis=2),
                              noise[:, :, 1] ^ 1, noise[:, :, 1])
    assert not (noise[:, :, None, :] == np.array(colors, dtype=np.uint8)[None, None]).all(axis=3).any()
    image[~kept] = noise[~kept]
    return image, colors, segm, kept


def clean(name):
    """(image uint8 [H, W, 3], {label: colour}, label map): a painted map without noise and its dictionary"""
    height, width, legend, seed, _ = PAINTED[name]
    colors = LEGENDS[legend]
    segm = blobs(height, width, len(colors), seed)
    return np.array(colors, dtype=np.uint8)[segm], {i: clr for i, clr in enumerate(colors)}, segm


def shifted_labels(name, shift=-3):
    """a label map whose labels start below zero, with its colour dictionary"""
    image, lut, segm = clean(name)
    return segm + shift, {lb + shift: clr for lb, clr in lut.items()}


def ambiguous_mask(labels, valid):
    """bool [H, W]: the pixels whose nearest valid pixels (all of those at the smallest squared distance) carry more than one label"""
    rows, cols = np.nonzero(valid)
    values = np.asarray(labels)[rows, cols]
    out = np.zeros(valid.shape, dtype=bool)
    xs = np.arange(valid.shape[1], dtype=np.int64)
    for y in range(valid.shape[0]):
        d2 = (y - rows[None, :]) ** 2 + (xs[:, None] - cols[None, :]) ** 2
        tied = d2 == d2.min(axis=1, keepdims=True)
        low = np.where(tied, values[None, :], values.max() + 1).min(axis=1)
        high = np.where(tied, values[None, :], values.min() - 1).max(axis=1)
        out[y] = low != high
    return out


def tied_labels_ok(result, labels, valid):
    """bool [H, W]: `result` is the label of ONE of the nearest valid pixels"""
    rows, cols = np.nonzero(valid)
    values = np.asarray(labels)[rows, cols]
    out = np.zeros(valid.shape, dtype=bool)
    xs = np.arange(valid.shape[1], dtype=np.int64)
    for y in range(valid.shape[0]):
        d2 = (y - rows[None, :]) ** 2 + (xs[:, None] - cols[None, :]) ** 2
        tied = d2 == d2.min(axis=1, keepdims=True)
        out[y] = (tied & (values[None, :] == np.asarray(result)[y][:, None])).any(axis=1)
    return out
