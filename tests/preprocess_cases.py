"""What tests/test_preprocess_emu.py (product host code on the lane emulator, device "cpu") and tests/test_preprocess_gpu.py (the MI355X, device "cuda") share:
the inputs, the temporary THINGS-shaped tree, the reduced towers and the checks themselves, written once against tests/preprocess_ref.py."""
import os
import pickle

import numpy as np
import torch

import preprocess_ref as R
from clip_vision_ref import Ref

TOWER = dict(hidden_size=640, intermediate_size=1280, num_hidden_layers=2, num_attention_heads=8, hidden_act="gelu", projection_dim=128)   # dim80_projection
SIZE = 28


def pil_images():
    """three images of different sizes: wide RGB, tall mode L (through .convert("RGB")), another wide RGB"""
    from PIL import Image
    rng = np.random.default_rng(0)
    u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    return [Image.fromarray(u8(40, 52, 3)), Image.fromarray(u8(60, 33)), Image.fromarray(u8(47, 61, 3))]


def check_presets(device):
    """each preset on the three images in one call against preprocess_ref under the normalisation bound, rows in input order; the second call hits the
    coefficient cache and is bit-identical; fp16 output within one unit in the last place; clip_image_processor also against transformers' own class"""
    from eeg_image_decode_amd import preprocess as P
    ims = pil_images()
    assert ims[1].mode == "L" and ims[1].size[1] > ims[1].size[0]
    for fn, ref, kw in ((P.open_clip_preprocess, R.open_clip_ref, dict(size=24)), (P.clip_image_processor, R.clip_image_processor_ref, dict(size=24)),
                        (P.vae_preprocess, R.vae_ref, dict(size=32))):
        out = fn(ims, device=device, **kw)
        n_tables = len(P._tables)
        again = fn(ims, device=device, **kw)
        assert len(P._tables) == n_tables and torch.equal(out, again) and out.dtype == torch.float32 and out.device.type == torch.device(device).type
        half = fn(ims, device=device, dtype=torch.float16, **kw).cpu()
        for i, im in enumerate(ims):
            q, sc, sh = ref(im, **kw)
            R.assert_normalized(out[i].cpu(), q, sc, sh)
            R.assert_normalized(half[i], q, sc, sh)
    # the two crop rules differ on the 61 x 47 image at 24 (31 - 24 = 7 is odd): the presets are not each other
    a, b = P.open_clip_preprocess(ims[2], size=24, device=device), P.clip_image_processor(ims[2], size=24, device=device)
    assert a.shape == b.shape == (1, 3, 24, 24) and not torch.equal(a, b) and torch.equal(a[..., :-1], b[..., 1:])
    # transformers' CLIPImageProcessor itself: its pixels are ours (recovered as integers, exactly), its floats within its own three fp32 roundings
    hf = R.hf_clip_image_processor(ims, size=24)
    ours = P.clip_image_processor(ims, size=24, device=device).cpu().numpy()
    mean, std = np.asarray(R.CLIP_MEAN)[None, :, None, None], np.asarray(R.CLIP_STD)[None, :, None, None]
    q_hf, q_ours = np.rint((hf.astype(np.float64) * std + mean) * 255), np.rint((ours.astype(np.float64) * std + mean) * 255)
    assert np.array_equal(q_hf, q_ours)
    assert (np.abs(hf.astype(np.float64) - ours) <= 2.0 ** -21 * (np.abs(q_ours / 255 / std) + np.abs(mean / std))).all()
    # raw integers, and the errors
    from eeg_image_decode_amd._lib import EegclipError
    raw = P.resize_crop_normalize(ims[0], (20, 30), rescale=None, device=device)
    assert np.array_equal(raw[0].cpu().numpy().astype(np.uint8).transpose(1, 2, 0), R.pil_resize(np.asarray(ims[0]), 20, 30, "bicubic"))
    for bad in (lambda: P.resize_crop_normalize(ims[0], 24, crop=(24, 40), device=device), lambda: P.resize_crop_normalize(ims, 24, device=device),
                lambda: P.resize_crop_normalize(torch.zeros(1, 3, 8, 8), 4, device=device), lambda: P.resize_crop_normalize(ims[0], 24, filter="lanczos", device=device),
                lambda: P.resize_crop_normalize(np.zeros((8, 8, 3), np.float32), 4, device=device)):
        try:
            bad()
        except EegclipError:
            continue
        raise AssertionError("no EegclipError")


def things_tree(root):
    """a THINGS-shaped tree: 2 classes x 2 PNGs of 52 x 40 per split, one subject's EEG files (4 images, 2 channels) -> the data_config dict"""
    from PIL import Image
    rng = np.random.default_rng(1)
    cfg = {"data_path": os.path.join(root, "eeg"), "img_directory_training": os.path.join(root, "train_images"), "img_directory_test": os.path.join(root, "test_images")}
    for key in ("img_directory_training", "img_directory_test"):
        for cls in ("00001_cat", "00002_sea_otter"):
            os.makedirs(os.path.join(cfg[key], cls))
            for j in range(2):
                Image.fromarray(rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)).save(os.path.join(cfg[key], cls, f"{cls}_{j:02d}.png"))
    os.makedirs(os.path.join(cfg["data_path"], "sub-01"))
    for split, reps in (("training", 4), ("test", 80)):
        d = {"preprocessed_eeg_data": rng.standard_normal((4, reps, 2, 10)), "ch_names": ["Pz", "Oz"], "times": np.linspace(-0.2, 0.39, 60)}
        with open(os.path.join(cfg["data_path"], "sub-01", f"preprocessed_eeg_{split}.npy"), "wb") as f:
            pickle.dump(d, f)
    return cfg


def encoders(device):
    from eeg_image_decode_amd import clip_text, clip_vision
    from test_clip_text_layout import _synthetic_vocab
    vocab, merges = _synthetic_vocab()
    tok = clip_text.BPETokenizer(vocab, merges)
    img = clip_vision.CLIPVisionEncoder(image_size=SIZE, dtype=torch.float16, seed=3, device=device, **TOWER)
    txt = clip_text.CLIPTextEncoder(128, 512, 2, 2, "gelu", 128, vocab_size=len(vocab), seed=4, device=device)
    return img, txt, tok


def check_feature_cache(root, device):
    """build_feature_cache writes the reference's file name and keys with unit-norm rows; img_features is image_features(open_clip_preprocess(..)) bit for bit
    and within tests/test_clip_vision_emu.py's 4e-3 (relative L2) of clip_vision_ref.Ref fed by preprocess_ref's pixels; EEGDataset keeps its error without
    encoders and builds the file with them"""
    from PIL import Image
    from eeg_image_decode_amd import datasets, preprocess
    cfg = things_tree(root)
    img_enc, txt_enc, tok = encoders(device)
    fn = datasets.build_feature_cache(cfg, True, img_enc, txt_enc, tok, features_dir=root)
    assert fn == os.path.join(root, "ViT-H-14_features_train.pt") and os.path.exists(fn)
    saved = torch.load(fn)
    assert sorted(saved) == ["img_features", "text_features"]
    tf, imf = saved["text_features"], saved["img_features"]
    assert tf.shape == (2, 128) and imf.shape == (4, 128) and tf.dtype == imf.dtype == torch.float32 and tf.device.type == "cpu"
    assert torch.allclose(tf.norm(dim=-1), torch.ones(2), atol=1e-5) and torch.allclose(imf.norm(dim=-1), torch.ones(4), atol=1e-5)
    texts, paths = datasets._listing(cfg["img_directory_training"])
    assert texts == ["This picture is cat", "This picture is sea_otter"] and len(paths) == 4
    ims = [Image.open(p) for p in paths]
    direct = datasets.image_features(preprocess.open_clip_preprocess(ims, size=SIZE, device=device), img_enc)
    assert torch.equal(direct.cpu(), imf)
    assert torch.equal(datasets.text_features(texts, txt_enc, tok).cpu(), tf) and not torch.equal(tf[0], tf[1])
    px = []
    for im in ims:
        q, sc, sh = R.open_clip_ref(im, size=SIZE)
        px.append(R.normalized(q, sc, sh)[0])
    want = Ref({k: v.cpu() for k, v in img_enc.state_dict().items()}, TOWER["num_attention_heads"], TOWER["hidden_act"])(
        torch.tensor(np.stack(px), dtype=torch.float32).half().float())["image_embeds"]
    want = want / want.norm(dim=-1, keepdim=True)
    rel = float((imf - want).norm() / want.norm())
    print(f"\n[rel-l2] img_features against Ref on preprocess_ref's pixels: {rel:.2e}", end=" ")
    assert rel < 4e-3
    # EEGDataset: today's error word for word without the encoders; with them the file is built on first use, then loaded
    kw = dict(subjects=["sub-01"], train=False, config=cfg, features_dir=root, device=device)
    missing = os.path.join(root, "ViT-H-14_features_test.pt")
    for partial in ({}, dict(image_encoder=img_enc, text_encoder=txt_enc)):
        try:
            datasets.EEGDataset(cfg["data_path"], **kw, **partial)
        except datasets.EegclipError as e:
            assert str(e) == (f"{missing} not found: the cached CLIP features are an input of this path (the reference creates them with open_clip "
                              "on first use, eegdatasets_leaveone.py:62-74)")
        else:
            raise AssertionError("EEGDataset did not raise")
        assert not os.path.exists(missing)
    ds = datasets.EEGDataset(cfg["data_path"], **kw, image_encoder=img_enc, text_encoder=txt_enc, tokenizer=tok)
    assert os.path.exists(missing) and ds.img_features.shape == (4, 128) and ds.text_features.shape == (2, 128) and len(ds) == 4
    assert torch.equal(ds.img_features.cpu(), torch.load(missing)["img_features"])
    try:
        datasets.EEGDataset(cfg["data_path"], classes=[0], **kw, image_encoder=img_enc, text_encoder=txt_enc, tokenizer=tok)
    except datasets.EegclipError as e:
        assert "classes / pictures" in str(e)
    else:
        raise AssertionError("classes= must stay rejected")
