"""Tools: the reference's examples/match.py on this library -- which images of a directory show the face of a reference image?

    python tools/match_dir.py REFERENCE IMAGE_DIR [--batch-size 1] [--threshold 0.5] [--gallery known.npz] [--out DIR]

The reference face goes into a FaceGallery under the name of its file (with --gallery, into the gallery saved there, beside
the names it already knows); every face found in IMAGE_DIR is then identified with one search per batch, and each match
under the threshold is printed as `path, name, confidence = distance`.  --out: the matched images with their faces drawn and
labelled are written there as JPEG.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import FaceGallery, extract_features, face_detection, image, vis      # noqa: E402

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference')
    ap.add_argument('image_dir')
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--gallery', default=None, help='a gallery written by FaceGallery.save: its names are searched too')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    reference = image.open_image(a.reference)
    faces = face_detection(reference)
    if len(faces) != 1:
        print('Reference image must have exactly one face.')
        return 1
    gallery = FaceGallery.load(a.gallery) if a.gallery else FaceGallery()
    gallery.add(os.path.splitext(os.path.basename(a.reference))[0], extract_features(reference, faces[0]))

    root = os.path.expanduser(a.image_dir)
    paths = sorted(os.path.join(root, f) for f in os.listdir(root) if f.lower().endswith(EXTENSIONS))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    for i in range(0, len(paths), max(a.batch_size, 1)):
        batch_paths = paths[i:i + max(a.batch_size, 1)]
        images = [image.open_image(p) for p in batch_paths]
        faces_per_image = face_detection(images)
        gallery.identify(faces_per_image, extract_features(images, faces_per_image), threshold=a.threshold)
        for path, img, faces in zip(batch_paths, images, faces_per_image):
            hits = [f for f in faces if 'distance' in f]
            for f in hits:
                print('%s, %s, confidence = %.2f' % (path, f['text'], f['distance']))
            if hits and a.out:
                from PIL import Image
                Image.fromarray(vis.vis_faces(img, hits, labels=True)).save(os.path.join(a.out, os.path.basename(path) + '.jpg'))
    return 0


if __name__ == '__main__':
    sys.exit(main())
