"""SDXLUNet's module layout on the meta device (no GPU, no weights): the state_dict keys and shapes of diffusers 0.30.0 UNet2DConditionModel with SDXL's config
(1,680 tensors, 2,567,463,684 parameters -- the published SDXL UNet size), and with the ip-adapter_sdxl_vit-h parameters (1,824 / 2,916,651,780), checked
against a key table written out here independently of the module."""
import pytest
import torch

from eeg_image_decode_amd._lib import EegclipError
from eeg_image_decode_amd.sdxl_unet import SDXLUNet

CH, LAYERS, TL, TEMB, X = (320, 640, 1280), 2, (1, 2, 10), 1280, 2048


def _lin(t, name, o, i, bias=True):
    t[name + ".weight"] = (o, i)
    if bias:
        t[name + ".bias"] = (o,)


def _norm(t, name, c):
    t[name + ".weight"] = (c,)
    t[name + ".bias"] = (c,)


def _conv(t, name, o, i, k):
    t[name + ".weight"] = (o, i, k, k)
    t[name + ".bias"] = (o,)


def _resnet(t, name, cin, cout):
    _norm(t, name + ".norm1", cin)
    _conv(t, name + ".conv1", cout, cin, 3)
    _lin(t, name + ".time_emb_proj", cout, TEMB)
    _norm(t, name + ".norm2", cout)
    _conv(t, name + ".conv2", cout, cout, 3)
    if cin != cout:
        _conv(t, name + ".conv_shortcut", cout, cin, 1)


def _transformer(t, name, c, layers, ip):
    _norm(t, name + ".norm", c)
    _lin(t, name + ".proj_in", c, c)
    for i in range(layers):
        b = f"{name}.transformer_blocks.{i}"
        for a, kv in (("attn1", c), ("attn2", X)):
            _lin(t, f"{b}.{a}.to_q", c, c, bias=False)
            _lin(t, f"{b}.{a}.to_k", c, kv, bias=False)
            _lin(t, f"{b}.{a}.to_v", c, kv, bias=False)
            _lin(t, f"{b}.{a}.to_out.0", c, c)
        if ip:
            _lin(t, f"{b}.attn2.processor.to_k_ip.0", c, X, bias=False)
            _lin(t, f"{b}.attn2.processor.to_v_ip.0", c, X, bias=False)
        for k in (1, 2, 3):
            _norm(t, f"{b}.norm{k}", c)
        _lin(t, f"{b}.ff.net.0.proj", 8 * c, c)
        _lin(t, f"{b}.ff.net.2", c, 4 * c)
    _lin(t, name + ".proj_out", c, c)


def key_table(ip):
    t = {}
    _conv(t, "conv_in", 320, 4, 3)
    _lin(t, "time_embedding.linear_1", TEMB, 320)
    _lin(t, "time_embedding.linear_2", TEMB, TEMB)
    _lin(t, "add_embedding.linear_1", TEMB, 2816)
    _lin(t, "add_embedding.linear_2", TEMB, TEMB)
    # down: DownBlock2D(320), CrossAttnDownBlock2D(640, 2 layers), CrossAttnDownBlock2D(1280, 10 layers, no downsampler)
    prev = 320
    for i, c in enumerate(CH):
        for j in range(LAYERS):
            _resnet(t, f"down_blocks.{i}.resnets.{j}", prev if j == 0 else c, c)
            if i > 0:
                _transformer(t, f"down_blocks.{i}.attentions.{j}", c, TL[i], ip)
        if i < 2:
            _conv(t, f"down_blocks.{i}.downsamplers.0.conv", c, c, 3)
        prev = c
    _resnet(t, "mid_block.resnets.0", 1280, 1280)
    _resnet(t, "mid_block.resnets.1", 1280, 1280)
    _transformer(t, "mid_block.attentions.0", 1280, 10, ip)
    # up: resnet inputs 2560, 2560, 1920 | 1920, 1280, 960 | 960, 640, 640
    ins = [(2560, 2560, 1920), (1920, 1280, 960), (960, 640, 640)]
    for i, c in enumerate((1280, 640, 320)):
        for j in range(LAYERS + 1):
            _resnet(t, f"up_blocks.{i}.resnets.{j}", ins[i][j], c)
            if i < 2:
                _transformer(t, f"up_blocks.{i}.attentions.{j}", c, (10, 2)[i], ip)
        if i < 2:
            _conv(t, f"up_blocks.{i}.upsamplers.0.conv", c, c, 3)
    _norm(t, "conv_norm_out", 320)
    _conv(t, "conv_out", 4, 320, 3)
    if ip:
        _lin(t, "encoder_hid_proj.image_projection_layers.0.image_embeds", 4 * X, 1024)
        _norm(t, "encoder_hid_proj.image_projection_layers.0.norm", X)
    return t


@pytest.mark.parametrize("ip, n_keys, n_params", [(False, 1680, 2_567_463_684), (True, 1824, 2_916_651_780)])
def test_state_dict_layout(ip, n_keys, n_params):
    m = SDXLUNet(device="meta", ip_adapter=ip)
    sd = m.state_dict()
    assert len(sd) == n_keys
    assert sum(v.numel() for v in sd.values()) == n_params
    table = key_table(ip)
    assert len(table) == n_keys
    assert {k: tuple(v.shape) for k, v in sd.items()} == table
    assert all(v.dtype == torch.float16 for v in sd.values())
    # a strict load of a dict built from the independent table
    m.load_state_dict({k: torch.empty(s, dtype=torch.float16, device="meta") for k, s in table.items()}, strict=True, assign=True)


def test_config_and_holders():
    m = SDXLUNet(device="meta", dtype=torch.bfloat16)
    c = m.config
    assert (c.in_channels, c.sample_size, c.time_cond_proj_dim, c.addition_time_embed_dim, c.cross_attention_dim) == (4, 128, None, 256, 2048)
    assert m.dtype == torch.bfloat16
    with pytest.raises(EegclipError):
        SDXLUNet(block_out_channels=(96, 192, 384), device="meta")                 # channels must be multiples of 64
    small = SDXLUNet(block_out_channels=(128, 256), transformer_layers_per_block=(1, 1), layers_per_block=1, ip_adapter=False,
                     down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), seed=3)
    again = SDXLUNet(block_out_channels=(128, 256), transformer_layers_per_block=(1, 1), layers_per_block=1, ip_adapter=False,
                     down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), seed=3)
    assert all(torch.equal(a, b) for a, b in zip(small.state_dict().values(), again.state_dict().values()))      # default init under the seed
    with pytest.raises(EegclipError):
        small(torch.zeros(1, 4, 8, 8), 1, torch.zeros(1, 77, 2048))                 # no CPU / eager path
