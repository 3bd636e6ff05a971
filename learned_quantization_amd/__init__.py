"""learned_quantization_amd -- MI355X-native (gfx950) learned-quantization hot path.

The nested-quantization fake-quant op (forward, STE, hand-written scale gradient), the three
custom loss terms and the scale update of anuunchin/learned-quantization, behind the
reference's own Python layer surface, executed by hand-written HIP kernels through the C ABI of
``include/lq_hip.h``.  See DESIGN.md / INTEGRATION.md.
"""
from .descriptor import (ORIENTATIONS, group_descriptor, group_geometry, groupwise_scale_shape, init_geometry, memory_descriptor, memory_order,
                         scale_shape)
from .layers import (default_kernel_storage, CustomConv2DLayer, CustomConv2DLayerNoBias, CustomDenseLayer, CustomQuantizedScaleLayer,
                     L2, MinValueConstraint, RandomNormal, SCALE_INIT, custom_layers_of, eps_float32, i8_conv_eligible, i8_dense_chain, i8_hardware, i8_hardware_eligible, init_scales, l2,
                     mx_conv_eligible, mx_dense_chain, mx_hardware, mx_hardware_eligible, mx_quant_stats, quant_stats, quantized_tensors, reset_layer_names)
from .losses import LossLog, SCCEDifference, SCCEInverse, SCCEMaxBin, sparse_categorical_crossentropy
from .ops import (difference_term, fq_backward_clip, fq_backward_group, fq_forward, fq_forward_clip, fq_forward_group, fq_fwd_bwd_fused, fq_scale_grad, fq_scale_grad_ste,
                  inverse_term, maxbin_term,
                  fq_backward_group_affine, fq_forward_group_affine, scale_init_group_minmax, GroupStats, group_stats, summarize_stats,
                  ELEMENT_FORMATS, check_element_format, fq_backward_mx, fq_forward_mx, scale_init_mx, MxStats, mx_stats, summarize_mx_stats,
                  MxOperand, mx_gemm, mx_gemm_quantize, mx_im2col_dims, mx_operand_decode, mx_operand_im2col, mx_operand_pack, mx_operand_quantize,
                  I8AffineOperand, I8Operand, check_i8_conv_operand_layer, check_i8_operand_layer, i8_gemm, i8_gemm_quantize, i8_operand_bytes, i8_operand_decode, i8_operand_im2col, i8_operand_pack, i8_operand_quantize,
                  my_custom_gradient, q_absmax_over_axis, q_minmax, q_pack, q_range_of, q_unique, q_unpack, quantized_integers, SCALE_INITS, scale_init_group)
from .optim import KerasAdam, ScaleAdam, apply_constraints, non_scale_parameters, scale_parameters
from .ddp import DataParallel, GradBucket
from .batch import BatchedScaleAdam, FakeQuantBatch
from .models import CIFARCNN, MNISTDense, ResNet18Like, ResNet50Like, build_model
from .data import augment_image, preprocess_for_validation
from .export import load_packed_parameters, save_compress_parameters, save_packed_parameters
from .tracking import AccuracyLossTrackingCallBack, GroupQuantTrackingCallback, MxQuantTrackingCallback, NestedScaleTrackingCallback

__version__ = "0.1.0"
