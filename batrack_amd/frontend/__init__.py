"""What batrack_amd provides of the reference's tracker front end (main/frontend) and of the steps of a frame around it.

  batrack_amd.frontend.corr.CorrBlock     the tracker's CorrBlock, fused: no correlation volume
  batrack_amd.frontend.corr.install       make the reference's unmodified md_tracker use it
  batrack_amd.frontend.track_iter.forward_iteration   the tracker's refinement loop around its transformers: tokens and state update
  batrack_amd.frontend.track_iter.sample_pos_embed    the position embedding of the tracks from two 1-D tables
  batrack_amd.frontend.track_iter.install             make the reference's md_tracker use both
  batrack_amd.frontend.update_former.forward          the update transformers: attention without the score matrix
  batrack_amd.frontend.update_former.attention        fused float32 attention over strided sequences
  batrack_amd.frontend.update_former.install          make the reference's UpdateFormer use it
  batrack_amd.frontend.tracker.forward                the tracker's window loop: depth range, window depth, 3-D feature maps, track features
  batrack_amd.frontend.tracker.embed_conv             `embedConv` with the Fourier embedding of (x, y, z) computed in the kernel
  batrack_amd.frontend.tracker.sample_features        each new track's features from its own frame
  batrack_amd.frontend.tracker.forward_frames         the single-window call on a `video.WindowFrames`: frames prepared and encoded once
  batrack_amd.frontend.tracker.install                make the reference's MDTracker use `forward`
  batrack_amd.frontend.encoder.encoder_head           the encoder's head: pyramid resize, 416 -> 256 conv, instance norm, 1 x 1, two launches
  batrack_amd.frontend.encoder.residual_block         one residual block of layer1..4: no normalised map in memory, five launches
  batrack_amd.frontend.encoder.encoder_trunk          layer1..4, the eight blocks: (a, b, c, d)
  batrack_amd.frontend.encoder.pack_block_weights     a block's weights in the layouts the kernels stage
  batrack_amd.frontend.encoder.packed_block           the same, cached per block
  batrack_amd.frontend.encoder.encoder_stem           the encoder's stem: 7 x 7 stride-2 conv1, instance norm, ReLU, normalised in place, three launches
  batrack_amd.frontend.encoder.pack_stem_weights      conv1's weights in the layout the kernel stages
  batrack_amd.frontend.encoder.packed_stem            the same with the bias, cached per module
  batrack_amd.frontend.encoder.stem_refusal           None, or what keeps a module's stem from being the reference's
  batrack_amd.frontend.encoder.forward                `BasicEncoder.forward` around them (encoder.DEVICE_STEM, encoder.DEVICE_LAYERS)
  batrack_amd.frontend.encoder.install                make the reference's BasicEncoder use `forward`
  batrack_amd.frontend.video.prepare_frames           the window's frames resized (exact coordinate), colours to [-1, 1], depth range: one launch
  batrack_amd.frontend.video.compute_sparse_tracks    `BATRACK._compute_sparse_tracks` around it
  batrack_amd.frontend.video.WindowFrames             the local window, each frame prepared and encoded once
  batrack_amd.frontend.video.install                  make the reference's BATRACK use `compute_sparse_tracks`
  batrack_amd.frontend.observe.window_observations tracker output -> the BA's targets and weights
  batrack_amd.frontend.keyframe.prune_keyframe       keyframe removal and edge pruning
  batrack_amd.frontend.patches.generate_patches      patch selection, depth initialisation and colours of a new frame
  batrack_amd.frontend.patches.image_gradient        the pooled gradient-magnitude map it ranks by
"""
