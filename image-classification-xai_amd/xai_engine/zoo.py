"""Classifier architectures for synthetic benchmarks and tests (seeded random weights -- there
is no network for checkpoints).  The hot path is model-agnostic: these exist only so that
bench.py can run BASELINE.json's named configurations (ResNet-50, ViT-B/16).

ResNet-50 is the standard v1.5 bottleneck network (stride on the 3x3 conv), the architecture
behind torchvision.models.resnet50; resnet101 / resnet152 / resnext101_64x4d are the deeper siblings the
reference harness instantiates (evaluatePerturbation.py:627-647: "R101", "R152", "RNXT"), same block with more
layers / grouped 3x3 convolutions, parameter names as in torchvision so that its state dicts load as they are.  ViT-B/16 follows the
layout of the reference's hooked model (util/attribution_methods/VIT_LRP/ViT_ig.py:57-253:
patch 16, dim 768, depth 12, 12 heads, qkv bias, LayerNorm eps 1e-6, class token, learned
position embedding) including its attention-map / attention-gradient hooks.
"""
import torch
import torch.nn as nn


# ------------------------------------------------------------------------------ ResNet-50
class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups          # ResNeXt: wider, grouped 3x3 (torchvision's rule)
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=False)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + idt)


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes=1000, width=64, groups=1, width_per_group=64):
        super().__init__()
        self.groups, self.base_width = groups, width_per_group
        self.inplanes = width
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make(width, layers[0], 1)
        self.layer2 = self._make(width * 2, layers[1], 2)
        self.layer3 = self._make(width * 4, layers[2], 2)
        self.layer4 = self._make(width * 8, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(width * 8 * 4, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make(self, planes, blocks, stride):
        down = None
        if stride != 1 or self.inplanes != planes * 4:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
        seq = [Bottleneck(self.inplanes, planes, stride, down, self.groups, self.base_width)]
        self.inplanes = planes * 4
        seq += [Bottleneck(self.inplanes, planes, groups=self.groups, base_width=self.base_width) for _ in range(1, blocks)]
        return nn.Sequential(*seq)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _frozen_resnet(seed, layers, num_classes, width, groups=1, width_per_group=64):
    torch.manual_seed(seed)
    m = ResNet(layers, num_classes, width, groups, width_per_group).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def resnet50(seed=0, num_classes=1000, width=64):
    return _frozen_resnet(seed, (3, 4, 6, 3), num_classes, width)


def resnet101(seed=0, num_classes=1000, width=64):
    """the reference's "R101" (evaluatePerturbation.py:627-633)"""
    return _frozen_resnet(seed, (3, 4, 23, 3), num_classes, width)


def resnet152(seed=0, num_classes=1000, width=64):
    """the reference's "R152" (:634-640; its table builds resnet101 and asks for ResNet152 weights -- here the architecture
    the weights belong to)"""
    return _frozen_resnet(seed, (3, 8, 36, 3), num_classes, width)


def resnext101_64x4d(seed=0, num_classes=1000, width=64):
    """the reference's "RNXT" (:641-647): 64 groups, 4 channels per group"""
    return _frozen_resnet(seed, (3, 4, 23, 3), num_classes, width, groups=64, width_per_group=4)


# ------------------------------------------------------------------------------ ViT-B/16 with hooks
class Attention(nn.Module):
    def __init__(self, dim, heads, qkv_bias=True):
        super().__init__()
        self.heads = heads
        self.scale = (dim // heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.attention_map = None
        self.attn_gradients = None
        self.output = None

    def save_attn_gradients(self, g):
        self.attn_gradients = g

    def get_output(self):
        """projected attention output of the last forward pass (reference ViT_new_timm.py:223-227,251): read by the InFlow rollout"""
        return self.output

    def get_attn_gradients(self):
        return self.attn_gradients

    def get_attention_map(self):
        return self.attention_map

    def forward(self, x, register_hook=False):
        B, N, D = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.heads, D // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1)
        self.attention_map = attn
        if register_hook and attn.requires_grad:
            attn.register_hook(self.save_attn_gradients)
        self.output = self.proj((attn @ v).transpose(1, 2).reshape(B, N, D))
        return self.output


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

        self.block_out = None
        self.input = self.input_plus_attn = self.mlp_val = None

    def get_block_out(self):
        """output of the last forward pass (reference ViT_new_timm.py:285,297-312): what `single_run(return_embeddings=True)` reads"""
        return self.block_out

    # the residual stream of the last forward pass (reference ViT_new_timm.py:276-283,297-312): what the InFlow rollout weighs
    def get_input(self):
        return self.input

    def get_input_plus_attn(self):
        return self.input_plus_attn

    def get_mlp_val(self):
        return self.mlp_val

    def forward(self, x, register_hook=False):
        self.input = x
        x = x + self.attn(self.norm1(x), register_hook)
        self.input_plus_attn = x
        y = self.mlp(self.norm2(x))
        self.mlp_val = y
        x = x + y
        self.block_out = x
        return x


class PatchEmbed(nn.Module):
    def __init__(self, patch, dim):
        super().__init__()
        self.patch_size = (patch, patch)
        self.proj = nn.Conv2d(3, dim, patch, stride=patch)

    def forward(self, x):
        """Non-overlapping patches: the stride-p p x p convolution IS a GEMM over (C*p*p)-vectors, and is run as one --
        same weights (`proj.weight` / `proj.bias`, so state dicts interchange with the reference's Conv2d), same sums.
        MIOpen has no tuned solver for this shape: in immediate mode its backward-data (the gradient with respect to the
        image, which every IG step needs) falls to a naive kernel at ~7 s per call."""
        p = self.patch_size[0]
        B, C, H, W = x.shape
        if H % p == 0 and W % p == 0:
            patches = x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // p) * (W // p), C * p * p)
            return nn.functional.linear(patches, self.proj.weight.reshape(self.proj.weight.shape[0], -1), self.proj.bias)
        return self.proj(x).flatten(2).transpose(1, 2)


class VisionTransformer(nn.Module):
    """Parameter names follow the reference's ViT_ig.py / timm (patch_embed.proj, blocks.N.attn.qkv,
    blocks.N.mlp.fc1 ...), so state dicts interchange."""

    def __init__(self, img=224, patch=16, dim=768, depth=12, heads=12, num_classes=1000):
        super().__init__()
        self.patch_embed = PatchEmbed(patch, dim)
        n = (img // patch) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, dim))
        self.pos_drop = nn.Identity()        # the reference's Dropout(p=0) (ViT_ig.py:175): TIS hangs its token-sampling hook here
        self.blocks = nn.ModuleList([Block(dim, heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.head = nn.Linear(dim, num_classes)
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x, register_hook=False):
        B = x.shape[0]
        x = self.patch_embed(x)
        x = self.pos_drop(torch.cat((self.cls_token.expand(B, -1, -1), x), dim=1) + self.pos_embed)
        for blk in self.blocks:
            x = blk(x, register_hook)
        return self.head(self.norm(x)[:, 0])


def vit_base_patch16_224(seed=0, **kw):
    torch.manual_seed(seed)
    m = VisionTransformer(**kw).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def vit_base_patch32_224(seed=0, **kw):
    """the reference's "VIT32" (evaluatePerturbation.py:654-659): patch 32, 7 x 7 patches"""
    return vit_base_patch16_224(seed, patch=32, **kw)


# ------------------------------------------------------------------------------ CLIP (ViT visual tower + causal text tower)
class Fp32LayerNorm(nn.LayerNorm):
    """LayerNorm of OpenAI's mixed precision: its parameters stay fp32, it computes in fp32 and returns the input's dtype"""

    def forward(self, x):
        return super().forward(x.float()).to(x.dtype)


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ClipAttention(nn.Module):
    """Multi-head self-attention over (L, N, D) tokens with the parameter names of nn.MultiheadAttention (in_proj_weight,
    in_proj_bias, out_proj), so that CLIP state dicts load as they are."""

    def __init__(self, dim, heads):
        super().__init__()
        self.embed_dim, self.num_heads = dim, heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)

    def forward(self, x, attn_mask=None):
        L, N, D = x.shape
        h, hd = self.num_heads, D // self.num_heads
        q, k, v = (t.reshape(L, N * h, hd).transpose(0, 1) for t in
                   nn.functional.linear(x, self.in_proj_weight, self.in_proj_bias).chunk(3, dim=-1))
        scores = torch.bmm(q * float(hd) ** -0.5, k.transpose(1, 2))
        if attn_mask is not None:
            scores = scores + attn_mask.to(dtype=scores.dtype, device=scores.device)
        out = torch.bmm(torch.softmax(scores, dim=-1), v).transpose(0, 1).reshape(L, N, D)
        return self.out_proj(out)


class ClipBlock(nn.Module):
    def __init__(self, dim, heads, attn_mask=None):
        super().__init__()
        self.attn = ClipAttention(dim, heads)
        self.ln_1 = Fp32LayerNorm(dim)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(dim, 4 * dim))
        self.mlp.add_module("gelu", QuickGELU())
        self.mlp.add_module("c_proj", nn.Linear(4 * dim, dim))
        self.ln_2 = Fp32LayerNorm(dim)
        self.attn_mask = attn_mask                      # a plain attribute, not a buffer: CLIP state dicts have no key for it

    def forward(self, x):
        x = x + self.attn(self.ln_1(x), self.attn_mask)
        return x + self.mlp(self.ln_2(x))


class ClipTransformer(nn.Module):
    def __init__(self, width, layers, heads, attn_mask=None):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*(ClipBlock(width, heads, attn_mask) for _ in range(layers)))

    def forward(self, x):
        return self.resblocks(x)


class ClipVisualTransformer(nn.Module):
    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, output_dim
        self.conv1 = nn.Conv2d(3, width, patch_size, stride=patch_size, bias=False)
        self.class_embedding = nn.Parameter(torch.randn(width) * width ** -0.5)
        self.positional_embedding = nn.Parameter(torch.randn((input_resolution // patch_size) ** 2 + 1, width) * width ** -0.5)
        self.ln_pre = Fp32LayerNorm(width)
        self.transformer = ClipTransformer(width, layers, heads)
        self.ln_post = Fp32LayerNorm(width)
        self.proj = nn.Parameter(torch.randn(width, output_dim) * width ** -0.5)

    def forward(self, x):
        x = self.conv1(x).flatten(2).transpose(1, 2)                                     # (N, grid * grid, width)
        x = torch.cat((self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1), x), dim=1)
        x = self.ln_pre(x + self.positional_embedding.to(x.dtype))
        x = self.transformer(x.transpose(0, 1)).transpose(0, 1)
        return self.ln_post(x[:, 0]) @ self.proj


class CLIP(nn.Module):
    """The CLIP of Radford et al. 2021 with a ViT visual tower, written from the published architecture.  Parameter names are
    OpenAI's (visual.conv1, visual.transformer.resblocks.N.attn.in_proj_weight, ..., token_embedding, text_projection,
    logit_scale), so a state_dict of `clip.load(...)` loads with strict=True.  Heads are width // 64 in both towers unless
    `vision_heads` or `transformer_heads` says otherwise (the head count is no parameter's shape, so a state dict loads either way)."""

    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length=77,
                 vocab_size=49408, transformer_width=512, transformer_heads=None, transformer_layers=12, vision_heads=None):
        super().__init__()
        self.context_length, self.vocab_size = context_length, vocab_size
        self.visual = ClipVisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                            vision_heads or max(1, vision_width // 64), embed_dim)
        self.transformer = ClipTransformer(transformer_width, transformer_layers, transformer_heads or max(1, transformer_width // 64),
                                           self.build_attention_mask())
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = Fp32LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.tensor(2.6592600369327779))              # log(1 / 0.07)
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        nn.init.normal_(self.text_projection, std=transformer_width ** -0.5)
        for tower in (self.visual.transformer, self.transformer):
            for blk in tower.resblocks:
                nn.init.normal_(blk.attn.in_proj_weight, std=tower.width ** -0.5)
                nn.init.normal_(blk.attn.out_proj.weight, std=(2 * tower.width * tower.layers) ** -0.5)
                nn.init.normal_(blk.mlp.c_fc.weight, std=(2 * tower.width) ** -0.5)
                nn.init.normal_(blk.mlp.c_proj.weight, std=(2 * tower.width * tower.layers) ** -0.5)

    def build_attention_mask(self):
        """the causal mask of the text tower: -inf above the diagonal"""
        return torch.full((self.context_length, self.context_length), float("-inf")).triu_(1)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        return self.visual(image.to(self.dtype))

    def encode_text(self, text):
        x = self.token_embedding(text).to(self.dtype) + self.positional_embedding.to(self.dtype)
        x = self.ln_final(self.transformer(x.transpose(0, 1)).transpose(0, 1)).to(self.dtype)
        return x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection     # the end-of-text token has the highest id

    def forward(self, image, text):
        img = nn.functional.normalize(self.encode_image(image), dim=-1)
        txt = nn.functional.normalize(self.encode_text(text), dim=-1)
        logits = self.logit_scale.exp() * img @ txt.t()
        return logits, logits.t()


def convert_weights_fp16(model):
    """OpenAI's mixed precision, in place: convolution, linear, attention and projection parameters in half; the LayerNorm
    parameters, the embeddings and logit_scale stay fp32 (the forward passes cast the embeddings)."""
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            m.weight.data = m.weight.data.half()
            if m.bias is not None:
                m.bias.data = m.bias.data.half()
        elif isinstance(m, ClipAttention):
            m.in_proj_weight.data = m.in_proj_weight.data.half()
            m.in_proj_bias.data = m.in_proj_bias.data.half()
        for name in ("text_projection", "proj"):
            p = getattr(m, name, None)
            if isinstance(p, nn.Parameter):
                p.data = p.data.half()
    return model


def clip_vit(seed=0, **sizes):
    """A frozen seeded CLIP of any size (the keywords of `CLIP`), fp32"""
    torch.manual_seed(seed)
    m = CLIP(**sizes).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def clip_vit_b16(seed=0):
    """OpenAI's ViT-B/16: the reference's "CLIP16" (generate_emap.py:42)"""
    return clip_vit(seed, embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16)


def clip_vit_b32(seed=0):
    """OpenAI's ViT-B/32: the reference's "CLIP32" (generate_emap.py:48)"""
    return clip_vit(seed, embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32)
