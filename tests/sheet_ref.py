"""The training loops' PNG sheets (main.py:203-226, 465-530) restated in numpy float32 + PIL: the checker of cgs_sheet_compose and of
cgs_amd.sheets.  Nothing here is imported by the package."""
import numpy as np

TILE, ROWS, LABEL_DY, FONT_SIZE = 64, 7, 12, 10


def to_u8(v):
    """np.uint8(255 * v) for a float32 array v: one float32 product, truncated."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    return (np.float32(255) * v).astype(np.uint8)


def tiles(A, B, Z):
    """The five image rows as float32 [n,64,64,3] each, every operation rounded to float32 in the reference's operand order
    (main.py:360-361, 470-474): A = u8 / 255, replaced = A * (1 - Z) + Z * B, injected = B * (1 - Z) + Z * A, Z on three channels."""
    a = A.astype(np.float32) / np.float32(255.0)
    b = B.astype(np.float32) / np.float32(255.0)
    z = np.asarray(Z, dtype=np.float32).reshape(len(A), TILE, TILE, 1)
    omz = np.float32(1) - z
    replaced = a * omz + z * b
    injected = b * omz + z * a
    for t in (a, b, omz, replaced, injected):
        assert t.dtype == np.float32
    return a, b, replaced, injected, np.concatenate((z, z, z), axis=-1)


def pixels(A, B, Z):
    """uint8 [7 * 64, 64 n, 3]: the segment sheet before the text (main.py:476-496)."""
    a, b, replaced, injected, z3 = tiles(A, B, Z)
    rows = [np.zeros_like(np.concatenate(a, axis=1))] * 2 + [np.concatenate(t, axis=1) for t in (a, b, replaced, injected, z3)]
    return to_u8(np.concatenate(rows, axis=0))


def draw(sheet, rows, n, font):
    """main.py:497-515 / 217-223: per (y, values) row str(round(value, 3)) of image i at (int(i * width / n), y), white."""
    from PIL import Image, ImageDraw
    img = Image.fromarray(sheet)
    d = ImageDraw.Draw(img)
    for y, values in rows:
        for i, value in enumerate(values):
            d.text((int(i * img.width / n), y), str(round(value, 3)), fill=(255, 255, 255), font=font)
    return np.array(img)


def segment_sheet(A, B, Z, Y, pred, negpred, replacevalue, injectvalue, font):
    """The finished segment sheet; the label rows are python floats (the reference's .tolist()), injectvalue None without inject."""
    rows = [Y, pred, negpred, replacevalue] + ([injectvalue] if injectvalue is not None else [])
    return draw(pixels(A, B, Z), [(LABEL_DY * k, v) for k, v in enumerate(rows)], len(A), font)


def critic_sheet(X, Y, pred, font):
    """main.py:211-226: the frames side by side, Y at y = 1, pred at y = int(1 + height / 2)."""
    sheet = np.uint8(np.concatenate(X, axis=1))
    return draw(sheet, [(1, Y), (int(1 + sheet.shape[0] / 2), pred)], len(X), font)


def column_hashes(sheet, row0=0):
    """SHA-256 of every 64-pixel image column of the sheet below row0."""
    import hashlib
    return [hashlib.sha256(np.ascontiguousarray(sheet[row0:, x:x + TILE]).tobytes()).hexdigest() for x in range(0, sheet.shape[1], TILE)]
