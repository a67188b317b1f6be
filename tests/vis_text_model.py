"""numpy restatement of the text part of terran/vis/pillow.py (draw_label) and of the DRAW_MASK primitive, on top of
tests/vis_raster.py.

Test infrastructure (the yardstick of tests/test_vis_text_cpu.py and tests/test_gpu_vis_text.py), written from Pillow's
documented behaviour and pinned black-box against the installed Pillow (test_vis_text_cpu.py's live check):

  mask(img, x0, y0, bitmap, rgb)   what draw.text places: an 8-bit coverage bitmap, top-left pixel at (x0, y0), blended
                                   per pixel as DIV255(in * (255 - m) + ink * m), clipped to the image
  draw_prims(frames, prims, masks) tests/vis_raster.draw_prims with DRAW_MASK (3) added
  RecordedFont                     the font of tests/golden/vis_text.npz: the metrics and coverage bitmaps the reference's
                                   font produced when the scenes were recorded, served through terran_amd.vis's font
                                   interface, so that the golden tests pin layout, order and blend whatever FreeType is
                                   installed where they run
  golden_scenes(path)              the scenes of tests/golden/vis_text.npz
  pillow_faces(...)                the reference's vis_faces with draw_label on the live Pillow, getsize(t) read as
                                   getbbox(t)[2:4]
"""
import string

import numpy as np

from tests import vis_raster as V

KIND_MASK = 3


def mask(img, x0, y0, bitmap, rgb):
    """Blend `bitmap` (h, w) uint8 coverage into img (H, W, 3) in place with its top-left pixel at (x0, y0)."""
    H, W = img.shape[:2]
    h, w = bitmap.shape
    ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ya >= yb or xa >= xb:
        return img
    m = bitmap[ya - y0:yb - y0, xa - x0:xb - x0].astype(np.int32)[..., None]
    v = img[ya:yb, xa:xb].astype(np.int32) * (255 - m) + np.asarray(rgb, np.int32) * m + 128
    img[ya:yb, xa:xb] = (((v >> 8) + v) >> 8).astype(np.uint8)
    return img


def draw_prims(frames, prims, masks=None):
    """Apply a PRIM_DT array to host frames (N, H, W, 3) in place, in order; a DRAW_MASK primitive reads its bitmap (rows
    packed, pitch x1 - x0 + 1) at byte offset `width` of `masks`."""
    for i, p in enumerate(prims):
        if int(p['kind']) != KIND_MASK:
            V.draw_prims(frames, prims[i:i + 1])
            continue
        assert int(p['rgba'][3]) == 255
        w, h, off = int(p['x1']) - int(p['x0']) + 1, int(p['y1']) - int(p['y0']) + 1, int(p['width'])
        assert off >= 0 and off + w * h <= len(masks)
        mask(frames[int(p['frame'])], int(p['x0']), int(p['y0']), masks[off:off + w * h].reshape(h, w), p['rgba'][:3])
    return frames


class RecordedFont:
    """terran_amd.vis's font interface over the tables of vis_text.npz; anything that was not recorded is a KeyError."""

    def __init__(self, tables, size):
        self.metrics, self.masks = tables
        self.size, self.key = size, ('recorded', size)

    def measure(self, text):
        return self.metrics[self.size, text]

    def mask(self, text, start):
        return self.masks[self.size, text, (float(start[0]), float(start[1]))]


def font_tables(z):
    metrics = {(int(s), str(t)): (int(w), int(h)) for s, t, (w, h) in zip(z['g_size'], z['g_text'], z['g_wh'])}
    masks, at = {}, 0
    for s, t, st, off, (h, w) in zip(z['m_size'], z['m_text'], z['m_start'], z['m_offset'], z['m_shape']):
        masks[int(s), str(t), (float(st[0]), float(st[1]))] = (z['m_data'][at:at + h * w].reshape(h, w),
                                                                 (int(off[0]), int(off[1])))
        at += int(h) * int(w)
    return metrics, masks


BOX_F32, BOX_INT, BOX_LIST = 0, 1, 2          # how a face's bbox is handed over: float32 array, int64 array, list of floats
TEXT_NONE, TEXT_STR, TEXT_INT, TEXT_FLOAT = 0, 1, 2, 3


def make_faces(bbox, box_kind, label_kind, name, track, text_kind, text):
    faces = []
    for b, bk, k, n, t, tk, tx in zip(bbox, box_kind, label_kind, name, track, text_kind, text):
        d = {'bbox': b.astype(np.float32) if bk == BOX_F32 else b.astype(np.int64) if bk == BOX_INT else [float(v) for v in b],
             'score': np.float32(0.9)}
        if k == 1:
            d['name'] = str(n)
        elif k == 2:
            d['track'] = int(t)
        if tk != TEXT_NONE:
            d['text'] = str(tx) if tk == TEXT_STR else int(str(tx)) if tk == TEXT_INT else float(str(tx))
        faces.append(d)
    return faces


def golden_scenes(path):
    """-> (npz, font tables, [scene dict]): seed, scale, base, expected, faces, colors of every scene."""
    from terran_amd import synth
    z = np.load(path)
    out = []
    for s in range(len(z['seeds'])):
        h, w = (int(v) for v in z['shapes'][s])
        seed = int(z['seeds'][s])
        base = synth.frames(seed, 1, h, w)[0]
        exp = base.copy().reshape(-1, 3)
        idx = np.cumsum(z['%d_didx' % s].astype(np.int64))
        exp[idx] = (exp[idx] + z['%d_dval' % s]).astype(np.uint8)
        faces = make_faces(*(z['%d_%s' % (s, k)] for k in ('bbox', 'box_kind', 'label_kind', 'name', 'track', 'text_kind',
                                                            'text')))
        out.append(dict(seed=seed, scale=float(z['scales'][s]), base=base, expected=exp.reshape(h, w, 3), faces=faces,
                        colors=z['%d_colors' % s]))
    return z, font_tables(z), out


def random_label_faces(rng, H, W, m):
    """(rng: random.Random) m faces at float32, integer and plain-float boxes on, over and beyond the edges of an H x W frame; half carry a
    `text` of printable ASCII (0-8 characters), a third a `track`, half a `name`."""
    faces = []
    for _ in range(m):
        x0, y0 = rng.uniform(-60, W + 10), rng.uniform(-40, H + 10)
        b = [x0, y0, x0 + rng.uniform(0, 60), y0 + rng.uniform(0, 60)]
        f = {'bbox': [np.array(b, np.float32), np.array(b).astype(np.int64), b][rng.randint(0, 2)]}
        r = rng.random()
        if r < 0.5:
            f['text'] = ''.join(rng.choice(string.printable[:95]) for _ in range(rng.randint(0, 8)))
        elif r < 0.85:
            f['track'] = rng.randint(0, 50)
        if rng.random() < 0.5:
            f['name'] = 'n%d' % rng.randint(0, 5)
        faces.append(f)
    return faces


# ---- the reference's vis_faces with labels, on the live Pillow --------------------------------------------------------
def pillow_font(size, names=('DejaVuSans-Bold', 'DroidSans-Bold')):
    from PIL import ImageFont
    for name in names:
        try:
            return ImageFont.truetype(name).font_variant(size=size)
        except IOError:
            continue
    return ImageFont.load_default()


def pillow_faces(img, faces, scale, colormap):
    """vis_faces of terran/vis/pillow.py on a copy of img: marker, then draw_label with getsize(t) = getbbox(t)[2:4]."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.array(img, np.uint8, copy=True))
    draw = ImageDraw.Draw(im, 'RGBA')
    for face in faces if isinstance(faces, (list, tuple)) else [faces]:
        rgb = tuple(colormap(face.get('name') or face.get('track')))
        draw.rectangle(list(face['bbox']), outline=rgb + (255,), width=int(3 * scale))
        text = face['text'] if face.get('text') is not None else \
            '#%s' % face['track'] if face.get('track') is not None else None
        if text is None:
            continue
        font = pillow_font(round(16 * scale))
        text = str(text)
        x, y = face['bbox'][:2]
        text_w = font.getbbox(text)[2]
        margin_w = font.getbbox('M')[2] * 0.2
        line_h = font.getbbox('Mq')[3]
        draw.rectangle([x, y, x + text_w + 3 * margin_w, y + line_h * 1.15], fill=rgb + (255,))
        draw.text([x + margin_w, y], text, font=font)
    return np.asarray(im)
