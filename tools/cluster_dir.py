"""Tools: who appears in the images of a directory?  match_dir.py's sibling without a reference face.

    python tools/cluster_dir.py IMAGE_DIR [--batch-size 1] [--threshold 0.5] [--min-samples 1] [--chips DIR]

Every face found in IMAGE_DIR is embedded; ONE `cluster_faces` call groups the embeddings on the device (DBSCAN, cosine
distance < threshold); each group is printed as `person K: n faces` followed by `  path, box` per face, faces that belong
to no group last.  --chips: one chip per group -- the face with the most neighbours -- is written there as person_K.jpg.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terran_amd import cluster_faces, extract_features, face_detection, image      # noqa: E402

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('image_dir')
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--min-samples', type=int, default=1)
    ap.add_argument('--chips', default=None)
    a = ap.parse_args()

    root = os.path.expanduser(a.image_dir)
    paths = sorted(os.path.join(root, f) for f in os.listdir(root) if f.lower().endswith(EXTENSIONS))
    faces, features, where = [], [], []
    for i in range(0, len(paths), max(a.batch_size, 1)):
        batch_paths = paths[i:i + max(a.batch_size, 1)]
        images = [image.open_image(p) for p in batch_paths]
        faces_per_image = face_detection(images)
        feats = extract_features(images, faces_per_image)
        for path, per_image, f in zip(batch_paths, faces_per_image, feats):
            faces.append(per_image)
            features.append(f)
            where.extend([path] * len(per_image))
    labels, representatives = cluster_faces(faces, features, threshold=a.threshold, min_samples=a.min_samples)
    flat = [face for per_image in faces for face in per_image]
    boxes = [tuple(int(v) for v in face['bbox']) for face in flat]
    for k in range(len(representatives)):
        members = [i for i, label in enumerate(labels) if label == k]
        print('person %d: %d faces' % (k, len(members)))
        for i in members:
            print('  %s, %s' % (where[i], boxes[i]))
    alone = [i for i, label in enumerate(labels) if label < 0]
    if alone:
        print('in no group: %d faces' % len(alone))
        for i in alone:
            print('  %s, %s' % (where[i], boxes[i]))
    if a.chips:
        from PIL import Image
        os.makedirs(a.chips, exist_ok=True)
        for k, i in enumerate(representatives):
            Image.fromarray(image.open_image(where[i])).crop(boxes[i]).save(os.path.join(a.chips, 'person_%d.jpg' % k))
    return 0


if __name__ == '__main__':
    sys.exit(main())
