from .train import (cuda_cast, point_wise_loss, load_checkpoint, checkpoint_save, is_multiple, weights_to_cpu, build_optimizer,  # noqa: F401
                    build_cosine_scheduler, build_dataloader)
from .pipeline import get_pointwise_preds, get_instances, group_dbscan, make_labels_consecutive  # noqa: F401
from .postprocess import propagate_preds  # noqa: F401
from .eval import (get_detections, get_detection_failures, evaluate_instance_segmentation, evaluate_no_partition,  # noqa: F401
                   evaluate_xy_partition, evaluate_z_partition, evaluate_no_partition_arrays, evaluate_xy_partition_arrays,
                   evaluate_z_partition_arrays, get_eval_components, get_segmentation_metrics, evaluate_forest, load_points)
from .hull import grid_points, get_hull, get_hull_buffer, get_coords_within_shape, get_cluster_means, ring_classify  # noqa: F401
from .segment import segment_forest, segment_from_pointwise, save_results, load_forest  # noqa: F401
