// Folded upsampler convs (hcp_conv3x3_up_fold_bf16): {mode (4 forward | 5 data gradient), M, N, K, 0, 1, 1, tile id, split-K, 8 + ring}.
