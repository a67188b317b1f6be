"""terran_amd -- MI355X-native (gfx950) detect + embed + pose path behind Terran's callables.

    from terran_amd import face_detection, extract_features, pose_estimation

mirror `terran.face_detection / extract_features / pose_estimation`
(terran/__init__.py:4-5): lazily-constructed `Detection`, `Recognition`, `Estimation`.
"""
from .facade import Detection, Recognition, Estimation          # noqa: F401
from .facade import TiledDetection                               # noqa: F401
from .facade import TiledEstimation                              # noqa: F401
from .retinaface import RetinaFace                                # noqa: F401
from .arcface import ArcFace                                      # noqa: F401
from .openpose import OpenPose, PoseOverflow                      # noqa: F401
from .gallery import FaceGallery, cluster_faces                   # noqa: F401
from .link import link_faces_poses, head_boxes                    # noqa: F401
from .tracking import PoseTracker, PoseTracking, pose_tracking    # noqa: F401
from .tracking import fill_pose_tracks, fill_face_tracks          # noqa: F401
from .vis import pose_masks, paint_poses, blur_poses, spotlight_poses, anonymize_poses    # noqa: F401

face_detection = Detection(lazy=True)
extract_features = Recognition(lazy=True)
pose_estimation = Estimation(lazy=True)
