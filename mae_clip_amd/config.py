"""Flag system, same names as the reference's config.py (config.py:1-36).

Changes vs the reference, all recorded in DESIGN.md:
  * model_name / image_embedding default to the ViT-B/16 of BASELINE.json
    (the reference default is timm resnet50 / 2048, config.py:15-16);
  * pretrained = False: hub weights are fetch-by-name and unavailable offline;
  * added: MAE head flags (mask_ratio, mae_weight, norm_pix_loss, decoder_*),
    text_layers, precision, seeds.
"""
import torch

debug = True
image_path = "/data/yuto/clip/OpenAI-CLIP/dataset/coco"
captions_path = "C:/Moein/AI/Datasets/Flicker-8k"
batch_size = 8
num_workers = 0
lr = 1e-3
weight_decay = 1e-3
patience = 2
factor = 0.5
epochs = 10
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

model_name = "vit_base_patch16_224"
image_embedding = 768
text_encoder_model = "distilbert-base-uncased"
text_embedding = 768
text_tokenizer = "distilbert-base-uncased"
max_length = 200

pretrained = False  # reference: True (hub download); no network here
trainable = True
temperature = 1.0
learnable_temperature = False   # True: CLIPModel trains log_temperature = ln(temperature) (one fp32 parameter,
                                # read by the loss kernels on the device); put it in a weight_decay = 0 group
# contrastive loss: "soft" = the reference's soft-target loss (CLIP.py:34-43, embeddings as they are),
# "infonce" = the OpenAI-CLIP loss (identity targets, symmetric cross-entropy), "siglip" = the pairwise
# sigmoid loss with a trained bias b (CLIPModel.logit_bias). The SigLIP paper initialises tau = 0.1
# (temperature = 0.1) with b = -10; log_temperature and logit_bias belong in a weight_decay = 0 group.
clip_loss = "soft"
normalize_embeddings = True     # "infonce" / "siglip": L2-normalise both embeddings first; "soft" never normalises
logit_bias_init = -10.0         # "siglip": initial b

# image size
size = 224

# for projection head; used for both image and text encoders
num_projection_layers = 1
projection_dim = 256
dropout = 0.1

# log
logdir = "./output/vit_mae_clip_amd"
checkpoints = "./output/vit_mae_clip_amd/checkpoints/"

# ---- added for the MAE head (BASELINE.json; HF ViTMAEConfig defaults)
mask_ratio = 0.75          # 0 => CLIP-only, no shuffle, no decoder (== reference path)
mae_weight = 1.0           # loss = clip + mae_weight * mae
norm_pix_loss = False
decoder_embed_dim = 512
decoder_depth = 8
decoder_num_heads = 16
decoder_mlp_ratio = 4.0

# ---- text encoder (DistilBertConfig defaults; C0 uses 2 layers)
text_layers = 6
text_heads = 12
text_hidden = 3072
text_vocab_size = 30522
text_max_position = 512
text_dropout = 0.1
text_attention_dropout = 0.1
text_trainable = False     # True: CLIPModel trains the text tower too (TextEncoder(trainable=True)); the
                           # reference's CLIPModel leaves it frozen (modules.py:35), which stays the default

# ---- numerics / determinism
precision = "bf16"         # "bf16" (perf), "fp8" (C4: e4m3/e5m2 stack GEMMs, bf16 elsewhere) or "fp32" (parity mode)
fp8_grad_format = "e4m3"   # fp8 mode: the dgrad GEMMs' gradient operand, "e4m3" (3 mantissa bits; the block / row
                           # scales give it the range) or "e5m2" (2 mantissa bits, wider range)
# fp8 mode: the attention (forward, backward) writes its output's fp8 blocks itself, else a standalone
# quantisation pass (A/B in DESIGN.md; MAECLIP_FP8_ATTN_Q8="10" / "11" / "00" for the A/B runs)
fp8_attn_q8 = tuple(c == "1" for c in __import__("os").environ.get("MAECLIP_FP8_ATTN_Q8", "11")[:2])
# fp8 mode: the MAE decoder stack on fp8 GEMMs too (with the producers writing the fp8
# operands, +1.9 % C4 fp8 and the same gradient error; MAECLIP_FP8_DECODER=0 for the
# bf16 decoder; A/B in DESIGN.md Round 6)
fp8_decoder = __import__("os").environ.get("MAECLIP_FP8_DECODER", "1") == "1"
mask_seed = 2
dropout_seed = 1234
# ---- training augmentation on the device (data.TrainAugment / data.train_augment_from_config): off by default,
# the reference's only transform is Resize + Normalize (dataset.py:44-58). The defaults are MAE's / torchvision's.
augment = False
augment_scale = (0.08, 1.0)        # RandomResizedCrop: crop area as a share of the image
augment_ratio = (3 / 4, 4 / 3)     # RandomResizedCrop: crop aspect ratio w / h, log-uniform
augment_flip_p = 0.5               # HorizontalFlip probability
augment_seed = 3
# ---- supervised evaluation of a pretrained image encoder (classifier.ClassifierModel): linear probe and fine-tuning.
# Read by ClassifierModel only; CLIPModel never looks at them.
num_classes = 1000
label_smoothing = 0.0              # F.cross_entropy's label_smoothing (MAE fine-tuning uses 0.1)
classifier_trainable_encoder = False   # False: linear probe (frozen encoder, only the head trains); True: fine-tuning
head_init_std = 0.02               # head.weight trunc-normal(std), head.bias zero (timm / MAE)
# ---- stochastic depth of the image encoder (timm drop_path_rate), training mode only: block i drops each residual
# branch of a sample with probability linspace(0, rate, depth)[i]. 0: off (today's launches). MAE fine-tunes ViT-B
# with 0.1, ViT-L / ViT-H with 0.2 / 0.3. Read by VisionTransformer; not available with precision "fp8".
# ClassifierModel applies it when its encoder trains (fine-tuning) and ignores it for the linear probe, whose
# frozen encoder has nothing to regularise; only an explicit ClassifierModel(drop_path_rate > 0) on a probe raises.
drop_path_rate = 0.0
# ---- Mixup / CutMix on the device (data.MixAugment); read by data.mix_augment_from_config() only. Both alphas 0:
# off (the default). MAE's / timm's fine-tuning recipe: mixup_alpha 0.8, cutmix_alpha 1.0, label_smoothing 0.1.
mixup_alpha = 0.0                  # Beta(alpha, alpha) of the mixup weight; 0: no mixup
cutmix_alpha = 0.0                 # Beta(alpha, alpha) of the cutmix area; 0: no cutmix
mix_prob = 1.0                     # probability that a draw mixes at all
mix_switch_prob = 0.5              # probability of cutmix when both alphas are > 0
mix_mode = "batch"                 # "batch": one draw per step; "elem": one per sample
mix_seed = 4
# ---- scheduling
side_stream = True         # frozen text tower || image encoder; weight-gradient GEMMs || the dgrad chain
# data parallel: encoder blocks per autograd Function, in forward order (the
# last size repeats; an int = equal chunks). Gradients of a chunk reach the
# bucketed all-reduce when its backward returns; the backward ends with the
# BOTTOM chunk, whose all-reduce cannot overlap any backward work, so it is
# the smallest (modules.chunk_bounds).
dp_encoder_chunk = (1, 2, 3, 6)
dp_decoder_chunk = 4       # data parallel: decoder blocks per autograd Function (overlapped by the encoder backward)
dp_grad_dtype = "fp32"     # data parallel gradient all-reduce: "fp32" (exact) or "bf16" (opt-in, half the bytes)
stack_microbatches = 2     # bf16 stacks: samples cut into this many micro-batches, each chain on its own stream
text_gemm_split = __import__("os").environ.get("MAECLIP_TEXT_SPLIT", "0") == "1"  # frozen text tower's GEMMs on the split plan (MAECLIP_GEMM_SK=1 scope; A/B knob)
wgrad_grouped = True       # all weight gradients of a stack in one grouped GEMM launch (maeclip_wgrad_grouped)
