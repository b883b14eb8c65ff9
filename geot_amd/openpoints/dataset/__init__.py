"""Dataloader-side ops on the GPU: the reference runs these on the CPU per scan
(openpoints/dataset/grid_sample.py, openpoints/dataset/tooth_semi/tooth_dataset.py:108-147), and the FixMatch training
batches its two loaders, transform lists and collation produce (fixmatch_batch), the validation loader's (val_batch), and
any transform list that keeps the point count as a per-view program (view_program; the supervised stage's batches:
supervised_batch); the batchers' per-item vertex sample drawn on the device instead of the host (sample_draw), and the transform lists' own
random draws -- view parameters, jitter noise, colour masks -- likewise (view_draw); the validation batches of test-time
voting, the `val` view and the `val` + `vote` view of one sample (vote_batch)."""
from .grid_sample import grid_subsampling  # noqa: F401
from .io import read_obj  # noqa: F401
from .scan_set import mesh_curvature  # noqa: F401
from .tooth_prep import pc_norm, prepare_sample  # noqa: F401
from .fixmatch_batch import (TOOTH_VIEW_KWARGS, DeviceScanSet, FixMatchBatcher, cloud_sample_batch, draw_view_params,  # noqa: F401
                             fixmatch_views)
from .sample_draw import DeviceDraws, ViewDrawHandle, cover_passes, sample_draw, sample_draw_cover  # noqa: F401
from .val_batch import ValBatcher, draw_val_sel  # noqa: F401
from .view_program import ViewProgram, pack_fixed_jobs, pack_program_jobs, view_program_views  # noqa: F401
from .view_draw import DrawLayout, view_draw, view_program_draw, view_program_views_drawn  # noqa: F401
from .supervised_batch import DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS, SupervisedBatcher  # noqa: F401
from .vote_batch import DEFAULT_VOTE, VoteBatcher  # noqa: F401
