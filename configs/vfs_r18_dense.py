# VFS ResNet-18 with the dense head: the per-position form of the frame-level similarity (DenseSimSiamHead: 1x1 ConvModules
# over the stage-4 feature map instead of average pool + Linear layers, cosine similarity per spatial position).  Channels
# as the frame-level head of vfs_r18.py (512 / 512 / 128 / 512); backbone, schedule and pipeline are that config's.
_norm = dict(type='SyncBN', requires_grad=True)
model = dict(
    type='SimSiamBaseTracker',
    backbone=dict(type='ResNet', depth=18, pretrained=None, out_indices=(3,), norm_cfg=_norm,
                  norm_eval=False, zero_init_residual=True),
    img_head=dict(type='DenseSimSiamHead', in_channels=512, norm_cfg=dict(type='SyncBN'),
                  num_projection_convs=3, projection_mid_channels=512, projection_out_channels=512,
                  num_predictor_convs=2, predictor_mid_channels=128, predictor_out_channels=512,
                  loss_feat=dict(type='CosineSimLoss', negative=False)))
train_cfg = dict(intra_video=True)
test_cfg = dict(precede_frames=20, topk=10, temperature=0.07, strides=(1, 2, 1, 1), out_indices=(2,),
                neighbor_range=24, with_first=True, with_first_neighbor=True, output_dir='eval_results')
# 2 clips x 4 frames per video, 32 videos per GPU
clip_len, num_clips, videos_per_gpu = 4, 2, 32
optimizer = dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=0.0001)
lr_config = dict(policy='CosineAnnealing', min_lr=0, by_epoch=False)
total_epochs = 100
dist_params = dict(backend='nccl')
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_bgr=False)
train_pipeline = [
    dict(type='DecordInit'),
    dict(type='SampleFrames', clip_len=1, frame_interval=0, num_clips=8, out_of_bound_opt='loop'),
    dict(type='Clip2Frame', clip_len=4),
    dict(type='DecordDecode'),
    dict(type='RandomResizedCrop', area_range=(0.2, 1.), same_across_clip=False, same_on_clip=False),
    dict(type='Resize', scale=(224, 224), keep_ratio=False),
    dict(type='Flip', flip_ratio=0.5, same_across_clip=False, same_on_clip=False),
    dict(type='Normalize', **img_norm_cfg),
    dict(type='FormatShape', input_format='NCTHW'),
    dict(type='Collect', keys=['imgs', 'label'], meta_keys=[]),
    dict(type='ToTensor', keys=['imgs', 'label']),
]
