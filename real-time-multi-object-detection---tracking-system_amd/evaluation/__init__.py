from .metrics import (COCO80_TO_91, HOTA_ALPHAS, build_confusion_matrix, coco_eval, coco_results, coco_stats, evaluate_detection, evaluate_tracking,
                      evaluate_tracking_hota, hota_combine, hota_eval, hota_record, load_coco, load_mot, measure_tracking_drift, mot_eval, mot_rows)
from .errors import analyze_detection_errors, detection_errors, format_confusion_matrix, format_error_table
from .stitch import correct_id_switches, stitch_tracks

__all__ = ["evaluate_detection", "evaluate_tracking", "build_confusion_matrix", "measure_tracking_drift", "coco_eval", "coco_stats",
           "mot_eval", "hota_eval", "hota_record", "hota_combine", "evaluate_tracking_hota", "HOTA_ALPHAS", "coco_results", "mot_rows", "load_coco", "load_mot", "COCO80_TO_91", "detection_errors", "analyze_detection_errors", "format_confusion_matrix",
           "format_error_table", "stitch_tracks", "correct_id_switches"]
