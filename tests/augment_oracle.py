"""What the input-pipeline tests share: the integer definition of include/ccnet_augment.h restated in NumPy (int64), the case
table, the seeded input builders and the guarded-buffer driver of the C ABI.

``cv2`` is not available where these tests run, so no fixture comes from the reference's own ``CSDataSet``: the oracle here is
the contract, and tests/test_augment_host.py cross-checks its image against torch's CPU ``F.interpolate`` away from exact ties.
Everything here is test infrastructure.
"""
import numpy as np

MEAN = (104.00698793, 116.66876762, 122.67891434)      # train.py's IMG_MEAN (B, G, R)
IGNORE = 255
DESC_INTS = 16
GUARD_BYTES = 256
GUARD_BYTE = 0xA5


def round_half_even_div(p, q):
    d, r2 = p // q, 2 * (p % q)
    return d + (1 if r2 > q or (r2 == q and d % 2 == 1) else 0)


def scaled_size(h, w, num, den):
    return max(1, round_half_even_div(h * num, den)), max(1, round_half_even_div(w * num, den))


def max_offsets(hs, ws, num, den, crop):
    hz, wz = scaled_size(hs, ws, num, den)
    return max(hz, crop[0]) - crop[0], max(wz, crop[1]) - crop[1]


def cityscapes_table(ignore=IGNORE):
    """dataset/datasets.py:146-151 restated for uint8 labels (independently of ccnet_amd.augment's table)"""
    ids = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15,
           31: 16, 32: 17, 33: 18}
    return np.array([ids.get(k, ignore) if k < 34 else k for k in range(256)], np.uint8)


def axis_taps(o, num, den, n_src):
    """(i0, i1, r) of sx = (o + 1/2) * den / num - 1/2 = i0 + r / (2 * num), clamped to the source, for an int64 array o"""
    o = np.asarray(o, np.int64)
    D = 2 * num
    t = (2 * o + 1) * den - num
    i0 = np.floor_divide(t, D)
    r = t - i0 * D
    neg = t < 0
    i0, r = np.where(neg, 0, i0), np.where(neg, 0, r)
    top = i0 >= n_src - 1
    i0, r = np.where(top, n_src - 1, i0), np.where(top, 0, r)
    return i0, np.minimum(i0 + 1, n_src - 1), r


def resized_levels(frame, num, den, Y, X):
    """The integer grey levels q (len(Y), len(X), 3) and the largest numerator, of the frame resized by num/den at rows Y and
    columns X of the scaled image (all inside it)."""
    Hs, Ws = frame.shape[:2]
    D = 2 * num
    j0, j1, ry = axis_taps(Y, num, den, Hs)
    i0, i1, rx = axis_taps(X, num, den, Ws)
    f = frame.astype(np.int64)
    rx, ry = rx[None, :, None], ry[:, None, None]
    top = f[j0][:, i0] * (D - rx) + f[j0][:, i1] * rx
    bot = f[j1][:, i0] * (D - rx) + f[j1][:, i1] * rx
    n = top * (D - ry) + bot * ry + D * D // 2
    return n // (D * D), int(n.max()) if n.size else 0


def augment_one(frame, label, sample, crop, mean=MEAN, ignore=IGNORE, table=None, source_rgb=True):
    """One sample by the contract: (float32 (3, crop_h, crop_w) in B, G, R, int64 (crop_h, crop_w)).  ``sample`` is
    (num, den, h_off, w_off, mirror)."""
    num, den, h_off, w_off, mirror = sample
    ch, cw = crop
    Hs, Ws = label.shape
    hz, wz = scaled_size(Hs, Ws, num, den)
    assert 0 <= h_off <= max(hz, ch) - ch and 0 <= w_off <= max(wz, cw) - cw
    xs = np.arange(cw)[::-1] if mirror else np.arange(cw)
    Y, X = h_off + np.arange(ch), w_off + xs
    iy, ix = np.nonzero(Y < hz)[0], np.nonzero(X < wz)[0]
    image = np.zeros((3, ch, cw), np.float32)
    out = np.full((ch, cw), ignore, np.int64)
    if iy.size and ix.size:
        q, top = resized_levels(frame, num, den, Y[iy], X[ix])
        assert top < 2 ** 32
        if source_rgb:
            q = q[:, :, ::-1]
        for c in range(3):
            image[c][np.ix_(iy, ix)] = q[:, :, c].astype(np.float32) - np.float32(mean[c])
        sy = np.minimum(Y[iy] * den // num, Hs - 1)
        sx = np.minimum(X[ix] * den // num, Ws - 1)
        v = label[sy][:, sx]
        out[np.ix_(iy, ix)] = (v if table is None else table[v]).astype(np.int64)
    return image, out


def augment_batch(frames, labels, samples, crop, **kw):
    pairs = [augment_one(f, l, s, crop, **kw) for f, l, s in zip(frames, labels, samples)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def make_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def make_label(h, w, seed, ids=tuple(range(34)) + (255,)):
    """Labels drawn from ``ids``; every id is present when the label has room for them."""
    rng = np.random.default_rng(seed + 1000)
    flat = rng.choice(np.array(ids, np.uint8), h * w)
    if h * w >= len(ids):
        flat[rng.permutation(h * w)[:len(ids)]] = ids
    return flat.reshape(h, w).astype(np.uint8)


# A sample is (Hs, Ws, num, den, h_off, w_off, mirror); an offset may be "max": the largest the contract allows.
# name: (crop, [samples], uses the Cityscapes table)
CASES = {}
for _tag, _num, _den in (("s05", 5, 10), ("s07", 7, 10), ("s10", 1, 1), ("s21", 21, 10)):
    # 20 x 30 to 16 x 16: 5/10 pads both axes (10 x 15), 7/10 the rows only (14 x 21), 1/1 and 21/10 none (20 x 30, 42 x 63)
    for _off in (0, "max"):
        for _mirror in (0, 1):
            CASES[f"{_tag}_{'far' if _off else 'origin'}{'_mirror' if _mirror else ''}"] = (
                (16, 16), [(20, 30, _num, _den, _off, _off, _mirror)], True)
CASES.update({
    # the i1 clamp and Ws - 1 = 0
    "src_1x1": ((16, 16), [(1, 1, 21, 10, 0, 0, 0)], True),
    "src_1x1_up": ((4, 4), [(1, 1, 1024, 1, "max", "max", 1)], False),
    "src_2x3": ((16, 16), [(2, 3, 21, 10, 0, 0, 1)], True),
    "src_2x3_up": ((5, 7), [(2, 3, 15, 2, "max", "max", 0)], False),
    "src_5x1": ((16, 16), [(5, 1, 21, 10, 0, 0, 0)], True),
    "src_5x1_down": ((2, 2), [(5, 1, 7, 10, "max", 0, 1)], False),
    # non-square crops; a row wider than one wave
    "crop_33x17": ((33, 17), [(20, 30, 21, 10, "max", 3, 1)], True),
    "crop_17x33": ((17, 33), [(20, 30, 21, 10, 2, "max", 0)], True),
    "crop_3x70": ((3, 70), [(20, 30, 21, 10, 5, 0, 1)], True),
    # the largest numerators (D = 2048): 1023/1024 keeps 5 x 6, 1024/1 gives 5120 x 6144 and the crop is its far corner
    "ratio_1023_1024": ((4, 4), [(5, 6, 1023, 1024, "max", "max", 0)], False),
    "ratio_1023_1024_pad": ((16, 16), [(5, 6, 1023, 1024, 0, 0, 1)], False),
    "ratio_1024_1": ((16, 16), [(5, 6, 1024, 1, "max", "max", 0)], False),
    "ratio_1024_1_mirror": ((16, 16), [(5, 6, 1024, 1, "max", "max", 1)], False),
    "ratio_1_1024": ((4, 4), [(20, 30, 1, 1024, 0, 0, 0)], False),            # everything collapses to one pixel
    # three frame sizes and scales in one launch; 3 * (551 + 35 + 99) = 2055 bytes of frames, the last one ending the buffer
    "batch_mixed": ((16, 16), [(19, 29, 7, 10, 0, "max", 0), (7, 5, 21, 10, 0, 0, 1), (9, 11, 1, 1, 0, 0, 0)], True),
    "batch_voc": ((12, 20), [(9, 11, 5, 10, 0, 0, 1), (19, 29, 16, 10, "max", "max", 0), (7, 5, 3, 2, 0, 0, 0)], False),
    # scale 1/1, no pad, no mirror: frame - mean and the table's labels
    "identity": ((16, 16), [(20, 30, 1, 1, 2, 5, 0)], True),
})


def build_case(name, seed=None):
    """(frames, labels, samples with their offsets resolved, crop, table) of a case; inputs are seeded by the case's place."""
    crop, raw, use_table = CASES[name]
    seed = list(CASES).index(name) * 16 if seed is None else seed
    frames, labels, samples = [], [], []
    for k, (hs, ws, num, den, h_off, w_off, mirror) in enumerate(raw):
        frames.append(make_frame(hs, ws, seed + k))
        labels.append(make_label(hs, ws, seed + k))
        mh, mw = max_offsets(hs, ws, num, den, crop)
        samples.append((num, den, mh if h_off == "max" else h_off, mw if w_off == "max" else w_off, mirror))
    return frames, labels, samples, crop, cityscapes_table() if use_table else None


def descriptors(frames, samples):
    """The int32 (B, 16) table of include/ccnet_augment.h for frames packed end to end"""
    desc, at = np.zeros((len(frames), DESC_INTS), np.int32), 0
    for b, (f, (num, den, h_off, w_off, mirror)) in enumerate(zip(frames, samples)):
        h, w = f.shape[:2]
        hz, wz = scaled_size(h, w, num, den)
        desc[b, :12] = [3 * at, at, h, w, w, num, den, hz, wz, h_off, w_off, mirror]
        at += h * w
    return desc


class GuardedBytes:
    """``nbytes`` of a back end of guarded_memory (HostMemory, DeviceMemory) starting on a 16-byte boundary, GUARD_BYTES of a
    fixed pattern in front and -- unless ``flush`` -- behind.  A ``flush`` buffer ends where its allocation ends and gives up
    the 16-byte alignment, which is how the packed frames of a real batch lie.  That is a layout, not a detector: the guard
    bands catch stray WRITES only, and a read past the end would go unseen here.  That the kernel reads no byte outside
    [frame_off, frame_off + ((Hs - 1) * pitch + Ws) * 3) follows from its byte-wide loads at clamped indices, by reading it."""

    def __init__(self, mem, nbytes, data=None, flush=False):
        self.mem, self.n = mem, nbytes
        lead = GUARD_BYTES + 16
        total = lead + nbytes + (0 if flush else GUARD_BYTES)
        self.raw, base = mem.new(total)
        # a flush buffer gives up the alignment instead of the position
        self.start = total - nbytes if flush else GUARD_BYTES + (-(base + GUARD_BYTES)) % 16
        self.ptr = base + self.start
        self.image = np.full(total, GUARD_BYTE, np.uint8)
        if data is not None:
            self.image[self.start:self.start + nbytes] = np.ascontiguousarray(data).view(np.uint8).ravel()
        mem.upload(self.raw, 0, self.image)

    def read(self, dtype):
        got = np.asarray(self.mem.download(self.raw))
        a, b = self.start, self.start + self.n
        intact = np.array_equal(got[:a], self.image[:a]) and np.array_equal(got[b:], self.image[b:])
        return got[a:b].copy().view(dtype), intact


def run_raw(lib, mem, frames, labels, samples, crop, table=None, mean=MEAN, ignore=IGNORE, source_rgb=True, desc=None):
    """One ccnet_augment_crop_u8 call on guarded buffers.  The packed frames and labels end flush with their allocations;
    the outputs start as NaN / -1.  Returns (code, images, labels, every guard band intact)."""
    B, (ch, cw) = len(frames), crop
    desc = np.ascontiguousarray(descriptors(frames, samples) if desc is None else desc, np.int32)
    fpack = np.concatenate([f.reshape(-1) for f in frames])
    lpack = np.concatenate([l.reshape(-1) for l in labels])
    fb = GuardedBytes(mem, fpack.size, fpack, flush=True)
    lb = GuardedBytes(mem, lpack.size, lpack, flush=True)
    db = GuardedBytes(mem, desc.nbytes, desc)
    tb = GuardedBytes(mem, 256, table) if table is not None else None
    img = GuardedBytes(mem, 4 * B * 3 * ch * cw, np.full(B * 3 * ch * cw, np.nan, np.float32))
    out = GuardedBytes(mem, 8 * B * ch * cw, np.full(B * ch * cw, -1, np.int64))
    code = lib.ccnet_augment_crop_u8(fb.ptr, fpack.size, lb.ptr, lpack.size, desc.ctypes.data, db.ptr,
                                     tb.ptr if tb else None, img.ptr, out.ptr, B, ch, cw, mean[0], mean[1], mean[2], ignore,
                                     int(source_rgb), mem.stream)
    images, ok_i = img.read(np.float32)
    lab, ok_l = out.read(np.int64)
    intact = ok_i and ok_l and all(b.read(np.uint8)[1] for b in (fb, lb, db) + ((tb,) if tb else ()))
    return code, images.reshape(B, 3, ch, cw), lab.reshape(B, ch, cw), intact


def assert_bit_exact(got_images, got_labels, want_images, want_labels):
    assert got_images.dtype == np.float32 and got_labels.dtype == np.int64
    assert np.array_equal(got_images.view(np.uint32), want_images.view(np.uint32)), \
        f"{int((got_images.view(np.uint32) != want_images.view(np.uint32)).sum())} image elements differ"
    assert np.array_equal(got_labels, want_labels), f"{int((got_labels != want_labels).sum())} labels differ"


def write_tiny_cityscapes(root, sizes, seed=40):
    """A Cityscapes-shaped tree of tiny PNG files under ``root`` (R, G, B frames, 8-bit grey id labels) and its list file;
    returns (list path, [(frame, label)])."""
    import os

    from PIL import Image
    lines, arrays = [], []
    os.makedirs(os.path.join(root, "img"))
    os.makedirs(os.path.join(root, "gt"))
    for k, (h, w) in enumerate(sizes):
        frame, label = make_frame(h, w, seed + k), make_label(h, w, seed + k)
        Image.fromarray(frame, "RGB").save(os.path.join(root, "img", f"f{k}_leftImg8bit.png"))
        Image.fromarray(label, "L").save(os.path.join(root, "gt", f"f{k}_gtFine_labelIds.png"))
        lines.append(f"img/f{k}_leftImg8bit.png gt/f{k}_gtFine_labelIds.png")
        arrays.append((frame, label))
    list_path = os.path.join(root, "train.lst")
    with open(list_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return list_path, arrays


WORKER_SEED = 4100


def seed_worker(worker_id):
    """``worker_init_fn``: the two generators the datasets draw from, seeded per worker"""
    import random
    random.seed(WORKER_SEED + worker_id)
    np.random.seed(WORKER_SEED + worker_id)


def replay_worker_draws(sizes, crop, batch_size, num_workers):
    """The AugmentParams per batch that ``num_workers`` workers seeded by :func:`seed_worker` draw for frames of ``sizes`` in
    order: a DataLoader gives batch k to worker k % num_workers, and each worker draws for its batches in turn."""
    import random

    from ccnet_amd import augment
    batches = [list(range(i, min(i + batch_size, len(sizes)))) for i in range(0, len(sizes), batch_size)]
    out = [None] * len(batches)
    keep = random.getstate(), np.random.get_state()
    for w in range(num_workers):
        seed_worker(w)
        for k in range(w, len(batches), num_workers):
            out[k] = [augment.draw_params(*sizes[i], crop) for i in batches[k]]
    random.setstate(keep[0])
    np.random.set_state(keep[1])
    return out
