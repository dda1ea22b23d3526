"""Python handle on one per-GPU render engine (libltk_hip.so).

PyTorch-ROCm is used only as plumbing here: device buffers (`torch.empty(...,
device="cuda")`) and their `data_ptr()`s.  All arithmetic runs in the HIP
library.  One `Engine` per GPU; sessions are sharded across engines by the
host - there is no cross-GPU traffic.
"""
from __future__ import annotations

import ctypes as C
import sys
import threading
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import HubertReq, LtkError, MtReq, NamedTensor, UlMergeReport, UlReq, W2lReq, WhisperReq  # noqa: F401


def _as_f32(a) -> np.ndarray:
    if hasattr(a, "detach"):  # torch tensor
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _conv_report_dict(rep: "_lib.ConvReport") -> dict:
    out = {name: getattr(rep, name) for name, _ in _lib.ConvReport._fields_}
    out["kernel"] = rep.kernel.decode()
    return out


class Engine:
    """avatars/wav2lip_avatar.py `model` handle + device-resident avatar banks."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.ltk_engine_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.max_frames = 0
        self.face_parse_size = None     # the image size load_face_parser built the parser for
        self._closed = False
        self._lock = threading.Lock()
        self._egress_open = set()       # egress sessions still open: closed with the engine
        # True: single-request wav2lip_infer calls may return with their pass in flight (knob DEFER).  Set by a caller whose frame
        # readers all go through this engine (paste_back*, egress_*) or through order_frames - the wav2lip plugin's handles do
        self.defer_handles = False

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        """Destroys the engine.  The handle is dropped with it: a later call on this object (a session's finalizer, a
        straggling paste) reaches the C ABI with a null engine and gets LTK_E_INVALID instead of touching freed memory."""
        if not self._closed:
            self._closed = True
            for sched in list(self.__dict__.get("_ltk_schedulers", {}).values()):     # scheduler.get_scheduler: stop the worker threads
                try:
                    sched.close()
                except Exception:
                    pass
            self.__dict__.pop("_ltk_schedulers", None)
            for sess in list(self._egress_open):
                try:
                    self.egress_close(sess)
                except Exception:
                    pass
            h, self._h = self._h, None
            self._lib.ltk_engine_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _lib.check(self._lib.ltk_engine_sync(self._h))

    @property
    def torch_device(self):
        """Where the plugin allocates the device buffers it hands to this engine."""
        import torch
        return torch.device("cuda", self.device)

    # ------------------------------------------------------------------ model
    @staticmethod
    def _named_tensors(state_dict: Dict[str, object]):
        keep = []
        arr = (NamedTensor * len(state_dict))()
        n = 0
        for name, t in state_dict.items():
            if name.endswith("num_batches_tracked"):
                continue
            a = _as_f32(t)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            nm = name.encode()
            keep.append((a, shape, nm))
            arr[n].name = nm
            arr[n].data = a.ctypes.data_as(C.POINTER(C.c_float))
            arr[n].ndim = a.ndim
            arr[n].shape = shape
            n += 1
        return arr, n, keep

    def load_wav2lip(self, state_dict: Dict[str, object], max_frames: int = 16):
        """wav2lip_avatar.py:59-70: `state_dict` = checkpoint["state_dict"] with any
        "module." prefix stripped (tensors or arrays)."""
        arr, n, keep = self._named_tensors(state_dict)
        _lib.check(self._lib.ltk_wav2lip_load(self._h, arr, n, int(max_frames)))
        self.max_frames = int(max_frames)
        del keep

    def load_musetalk(self, unet_sd: Dict[str, object], vae_sd: Dict[str, object], max_frames: int = 16, fp8: bool = False,
                      fp8_act_scale: float = 0.0):
        """musetalk_avatar.py:57-67: diffusers-named state dicts of the U-Net (models/musetalkV15/unet.pth) and of
        the sd-vae AutoencoderKL (post_quant_conv.*, decoder.*).  fp8: ResnetBlock2D 3x3 convs on e4m3 operands
        (BASELINE configs[4])."""
        if fp8:
            _lib.check(self._lib.ltk_musetalk_set_fp8(self._h, 1, float(fp8_act_scale)))
        ua, un, k1 = self._named_tensors(unet_sd)
        va, vn, k2 = self._named_tensors(vae_sd)
        _lib.check(self._lib.ltk_musetalk_load(self._h, ua, un, va, vn, int(max_frames)))
        self.mt_max_frames = int(max_frames)
        del k1, k2

    # ------------------------------------------------------------------ avatars
    def register_avatar(self, face_list: Sequence[np.ndarray], frame_list: Sequence[np.ndarray],
                        coord_list: Sequence[Sequence[int]]) -> int:
        """Upload (frame_list_cycle, face_list_cycle, coord_list_cycle) as
        load_avatar returns them (wav2lip_avatar.py:72-88)."""
        # a packed bank (livetalking_amd/bank.py) hands over its contiguous mmap sections: no re-stacking, one H2D copy each
        faces = getattr(face_list, "packed", None)
        fulls = getattr(frame_list, "packed", None)
        faces = np.ascontiguousarray(np.stack(face_list) if faces is None else faces, dtype=np.uint8)
        fulls = np.ascontiguousarray(np.stack(frame_list) if fulls is None else fulls, dtype=np.uint8)
        coords = np.ascontiguousarray(np.asarray(coord_list, dtype=np.int32).reshape(-1, 4))
        n = faces.shape[0]
        if faces.shape[1:] != (256, 256, 3) or fulls.shape[0] != n or coords.shape[0] != n or fulls.shape[3] != 3:
            raise ValueError("avatar bank shapes: faces (n,256,256,3), frames (n,H,W,3), coords (n,4)")
        aid = C.c_int()
        _lib.check(self._lib.ltk_avatar_register(self._h, faces.ctypes.data, fulls.ctypes.data, coords.ctypes.data,
                                                 n, fulls.shape[1], fulls.shape[2], C.byref(aid)))
        return aid.value

    def release_avatar(self, avatar_id: int):
        _lib.check(self._lib.ltk_avatar_release(self._h, int(avatar_id)))

    # ------------------------------------------------------------------ hot path
    def mel_step(self, pcm: np.ndarray, win_start: Sequence[int], d_out_ptr: int, stream: int = 0):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        ws = np.ascontiguousarray(win_start, dtype=np.int32)
        _lib.check(self._lib.ltk_mel_step(self._h, pcm.ctypes.data, pcm.shape[0], ws.ctypes.data, ws.shape[0],
                                          C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def wav2lip_infer(self, reqs: Sequence[tuple], stream: int = 0):
        """reqs: (avatar_id, index, batch, d_mel_ptr, d_pred_ptr) per session; each
        session's uint8 frames [batch][256][256][3] land in its own d_pred."""
        arr = (W2lReq * len(reqs))()
        for i, (aid, index, batch, mel_ptr, pred_ptr) in enumerate(reqs):
            arr[i].avatar = int(aid)
            arr[i].index = int(index)
            arr[i].batch = int(batch)
            arr[i].d_mel = C.c_void_p(mel_ptr)
            arr[i].d_pred = C.c_void_p(pred_ptr)
        if len(reqs) == 1 and self.defer_handles:
            # a lone request may return with its pass in flight (knob DEFER, include/ltk.h: ltk_wav2lip_infer_deferred; the engine
            # decides).  The engine's own consumers (paste_back*, egress_*) order themselves behind that pass; every other reader of
            # the frames goes through order_frames first - which is what `defer_handles` promises
            deferred = C.c_int(0)
            _lib.check(self._lib.ltk_wav2lip_infer_deferred(self._h, arr, 1, C.c_void_p(stream), 0, C.byref(deferred)))
            return bool(deferred.value)          # True: the frames' pass is in flight, the caller wraps / orders its readers
        _lib.check(self._lib.ltk_wav2lip_infer(self._h, arr, len(reqs), C.c_void_p(stream)))
        return False

    def current_stream(self) -> int:
        """torch's current stream on this engine's GPU as a handle (0 = the default stream, also without torch)."""
        torch = sys.modules.get("torch")
        return int(torch.cuda.current_stream(self.device).cuda_stream) if torch is not None else 0

    def order_frames(self, d_pred_ptr: int, nbytes: int, stream: Optional[int] = None):
        """Makes `stream` (default: torch's current stream on this engine's GPU; 0 = the default stream) wait, on the GPU, for the
        deferred pass that writes [d_pred_ptr, d_pred_ptr + nbytes), if one is in flight.  No host wait.  The wait is issued when
        the frames are READ instead of with every call: a wait given to torch's stream at every call sat in a hardware queue for the
        length of every pass and cost more than the deferral gains (profiles/defer_ab.txt)."""
        if stream is None:
            stream = self.current_stream()
        _lib.check(self._lib.ltk_wav2lip_order_stream(self._h, C.c_void_p(d_pred_ptr), int(nbytes), C.c_void_p(stream)))

    def defer_stats(self) -> dict:
        """Knob DEFER (include/ltk.h): calls that returned with their pass outstanding / the most passes outstanding at such a return /
        passes outstanding now."""
        d, m, o = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        _lib.check(self._lib.ltk_wav2lip_defer_stats(self._h, C.byref(d), C.byref(m), C.byref(o)))
        return {"deferred": int(d.value), "max_outstanding": int(m.value), "outstanding": int(o.value)}

    def paste_back(self, avatar_id: int, idx: int, d_pred_ptr: int, out: np.ndarray, stream: int = 0):
        """out: C-contiguous uint8 (H,W,3) host array, filled in place."""
        _lib.check(self._lib.ltk_paste_back(self._h, int(avatar_id), int(idx), C.c_void_p(d_pred_ptr),
                                            out.ctypes.data, 0, C.c_void_p(stream)))

    def paste_back_batch(self, avatar_id: int, idx: Sequence[int], d_pred_ptr: int, out_ptr: int, stream: int = 0):
        """n = len(idx) composites (n contiguous device predictions) into host memory at out_ptr [n][H][W][3] (pinned for
        the PCIe rate): one device-to-host copy, one synchronisation (include/ltk.h: ltk_paste_back_batch)."""
        arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int32))
        _lib.check(self._lib.ltk_paste_back_batch(self._h, int(avatar_id), arr.ctypes.data, C.c_void_p(d_pred_ptr), int(arr.size),
                                                  C.c_void_p(out_ptr), C.c_void_p(stream)))

    def paste_back_device(self, avatar_id: int, idx: int, d_pred_ptr: int, d_out_ptr: int, stream: int = 0):
        _lib.check(self._lib.ltk_paste_back(self._h, int(avatar_id), int(idx), C.c_void_p(d_pred_ptr),
                                            C.c_void_p(d_out_ptr), 1, C.c_void_p(stream)))

    # ------------------------------------------------------------------ musetalk
    def register_musetalk_avatar(self, latents: Sequence[np.ndarray], frame_list: Sequence[np.ndarray], coord_list,
                                 mask_list: Sequence[np.ndarray], mask_coords_list) -> int:
        """(frame_list_cycle, mask_list_cycle, coord_list_cycle, mask_coords_list_cycle, input_latent_list_cycle) as
        musetalk_avatar.load_avatar returns them (musetalk_avatar.py:69-91)."""
        lat = np.ascontiguousarray(np.concatenate([_as_f32(x).reshape(1, 8, 32, 32) for x in latents]), dtype=np.float32)
        fulls = getattr(frame_list, "packed", None)
        fulls = np.ascontiguousarray(np.stack(frame_list) if fulls is None else fulls, dtype=np.uint8)
        fb = np.ascontiguousarray(np.asarray(coord_list, dtype=np.int32).reshape(-1, 4))
        cb = np.ascontiguousarray(np.asarray(mask_coords_list, dtype=np.int32).reshape(-1, 4))
        n = lat.shape[0]
        flat = [np.ascontiguousarray(m, dtype=np.uint8).reshape(-1) for m in mask_list]
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum([f.size for f in flat])
        masks = np.ascontiguousarray(np.concatenate(flat))
        aid = C.c_int()
        _lib.check(self._lib.ltk_musetalk_avatar_register(self._h, lat.ctypes.data, fulls.ctypes.data, fb.ctypes.data, cb.ctypes.data,
                                                          masks.ctypes.data, offs.ctypes.data, n, fulls.shape[1], fulls.shape[2],
                                                          C.byref(aid)))
        return aid.value

    def musetalk_infer(self, reqs: Sequence[tuple], stream: int = 0):
        """reqs: (avatar_id, index, batch, d_feat_ptr fp32 [batch][50][384], d_pred_ptr uint8 [batch][256][256][3])."""
        arr = (MtReq * len(reqs))()
        for i, (aid, index, batch, feat_ptr, pred_ptr) in enumerate(reqs):
            arr[i].avatar = int(aid); arr[i].index = int(index); arr[i].batch = int(batch)
            arr[i].d_feat = C.c_void_p(feat_ptr); arr[i].d_pred = C.c_void_p(pred_ptr)
        _lib.check(self._lib.ltk_musetalk_infer(self._h, arr, len(reqs), C.c_void_p(stream)))

    def paste_blend(self, avatar_id: int, idx: int, d_pred_ptr: int, out: np.ndarray, stream: int = 0):
        _lib.check(self._lib.ltk_paste_blend(self._h, int(avatar_id), int(idx), C.c_void_p(d_pred_ptr), out.ctypes.data, 0,
                                             C.c_void_p(stream)))

    # ------------------------------------------------------------------ ultralight
    def register_ultralight_avatar(self, state_dict: Dict[str, object], face_list: Sequence[np.ndarray], frame_list: Sequence[np.ndarray],
                                   coord_list, max_frames: int = 16) -> int:
        """(model, frame_list_cycle, face_list_cycle, coord_list_cycle) as ultralight_avatar.load_avatar returns them
        (ultralight_avatar.py:63-81): `state_dict` = torch.load(ultralight.pth) (tensors or arrays), 168x168 BGR faces, full frames,
        (x1, y1, x2, y2) boxes.  The model is per avatar, so it is registered with the bank."""
        faces = np.ascontiguousarray(np.stack(face_list), dtype=np.uint8)
        fulls = getattr(frame_list, "packed", None)
        fulls = np.ascontiguousarray(np.stack(frame_list) if fulls is None else fulls, dtype=np.uint8)
        coords = np.ascontiguousarray(np.asarray(coord_list, dtype=np.int32).reshape(-1, 4))
        n = faces.shape[0]
        if faces.shape[1:] != (168, 168, 3) or fulls.ndim != 4 or fulls.shape[0] != n or coords.shape[0] != n or fulls.shape[3] != 3:
            raise ValueError("ultralight avatar bank shapes: faces (n,168,168,3), frames (n,H,W,3), coords (n,4)")
        arr, nt, keep = self._named_tensors(state_dict)
        aid = C.c_int()
        _lib.check(self._lib.ltk_ultralight_avatar_register(self._h, arr, nt, faces.ctypes.data, fulls.ctypes.data, coords.ctypes.data,
                                                            n, fulls.shape[1], fulls.shape[2], int(max_frames), C.byref(aid)))
        del keep
        return aid.value

    def ultralight_infer(self, reqs: Sequence[tuple], stream: int = 0):
        """reqs: (avatar_id, index, batch, d_feat_ptr fp32 [batch][16][32][32], d_pred_ptr uint8 [batch][160][160][3])."""
        arr = (UlReq * len(reqs))()
        for i, (aid, index, batch, feat_ptr, pred_ptr) in enumerate(reqs):
            arr[i].avatar = int(aid); arr[i].index = int(index); arr[i].batch = int(batch)
            arr[i].d_feat = C.c_void_p(feat_ptr); arr[i].d_pred = C.c_void_p(pred_ptr)
        _lib.check(self._lib.ltk_ultralight_infer(self._h, arr, len(reqs), C.c_void_p(stream)))

    def ultralight_infer_merged(self, reqs: Sequence[tuple], mode: int = 0, stream: int = 0, report: bool = False):
        """ultralight_infer with the requests' passes merged (include/ltk.h: ltk_ultralight_infer_merged): one launch sequence per pass
        of the call plan instead of one per request.  mode 0: the rule (knob UL_GROUPED decides for several avatars), 1: per avatar,
        2: grouped.  report=True -> {"passes": [(path, frames, avatar)], "avatars", "grouped", "frames"} of what was launched."""
        arr = (UlReq * len(reqs))()
        for i, (aid, index, batch, feat_ptr, pred_ptr) in enumerate(reqs):
            arr[i].avatar = int(aid); arr[i].index = int(index); arr[i].batch = int(batch)
            arr[i].d_feat = C.c_void_p(feat_ptr); arr[i].d_pred = C.c_void_p(pred_ptr)
        rep = UlMergeReport() if report else None
        _lib.check(self._lib.ltk_ultralight_infer_merged(self._h, arr, len(reqs), int(mode), C.c_void_p(stream),
                                                         C.byref(rep) if report else None))
        if not report:
            return None
        n = min(rep.n_passes, _lib.UL_MERGE_MAX_PASSES)
        return {"passes": [(rep.path[i], rep.nf[i], rep.avatar[i]) for i in range(n)], "n_passes": rep.n_passes, "avatars": rep.n_avatars,
                "grouped": rep.grouped, "frames": rep.frames}

    def ultralight_info(self) -> dict:
        """The Ultralight arena: frames per pass, bytes, bytes per frame, and whether the grouped path is built."""
        fr, gr = C.c_int(0), C.c_int(0)
        ab, bf = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self._lib.ltk_ultralight_info(self._h, C.byref(fr), C.byref(ab), C.byref(bf), C.byref(gr)))
        return {"frames": fr.value, "bytes": ab.value, "bytes_per_frame": bf.value, "grouped": bool(gr.value)}

    @property
    def ul_max_frames(self) -> int:
        """Frames one Ultralight pass carries (the scheduler's limit for kind "ultralight"); 0 before the first avatar."""
        return min(self.ultralight_info()["frames"], 256)

    @staticmethod
    def ul_merge_plan(reqs: Sequence[tuple], cap: int, mode: int = 0, grouped_available: bool = True, grouped_knob: int = -1):
        """ltk_debug_ul_merge_plan (no GPU, no engine): reqs = (avatar, batch) -> [(path, avatar, frames, [(request, first frame of the
        request, count, first frame in the pass)])]."""
        lib = _lib.load()
        n = len(reqs)
        av = (C.c_int * max(n, 1))(*[int(a) for a, _ in reqs])
        nb = (C.c_int * max(n, 1))(*[int(b) for _, b in reqs])
        total = sum(max(int(b), 0) for _, b in reqs)
        mp = max(1, total // max(int(cap), 1) + n + 1)
        ms = mp + n + 1
        pp, pa, pn = (C.c_int * mp)(), (C.c_int * mp)(), (C.c_int * mp)()
        sp, sr, sf, sc, sa = ((C.c_int * ms)() for _ in range(5))
        npass, nspan = C.c_int(0), C.c_int(0)
        _lib.check(lib.ltk_debug_ul_merge_plan(av, nb, n, int(cap), int(mode), int(bool(grouped_available)), int(grouped_knob),
                                               pp, pa, pn, mp, C.byref(npass), sp, sr, sf, sc, sa, ms, C.byref(nspan)))
        plan = [(pp[i], pa[i], pn[i], []) for i in range(npass.value)]
        for j in range(nspan.value):
            plan[sp[j]][3].append((sr[j], sf[j], sc[j], sa[j]))
        return plan

    @staticmethod
    def ul_program(fuse: int = -1, max_ops: int = 96, max_bufs: int = 12) -> dict:
        """ltk_debug_ultralight_program (no GPU, no engine): the launches of a per-avatar pass with the fused inverted residual off (0),
        on (1) or as knob UL_FUSE_IR stands (-1) -> {"ops": [dict of include/ltk.h ltk_ul_op_info's fields], "buf_halfs": [...]}."""
        ops = (_lib.UlOpInfo * max(int(max_ops), 1))()
        halfs = (C.c_uint64 * max(int(max_bufs), 1))()
        n_ops, n_bufs = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().ltk_debug_ultralight_program(int(fuse), ops, int(max_ops), C.byref(n_ops), halfs, int(max_bufs), C.byref(n_bufs)))
        fields = [n for n, _ in _lib.UlOpInfo._fields_]
        return {"ops": [{n: (getattr(o, n).decode() if n == "name" else getattr(o, n)) for n in fields} for o in ops[:n_ops.value]],
                "buf_halfs": [int(h) for h in halfs[:n_bufs.value]]}

    def ul_gconv_f16(self, d_x_ptr: int, N, H, W, Cin, weight: np.ndarray, sets: Sequence[int], k: int = 1, stride: int = 1, pad: int = 0,
                     scale=None, shift=None, d_res_ptr: int = 0, relu: bool = False, d_y_ptr: int = 0, views: Optional[dict] = None):
        """The grouped dense conv on its own (include/ltk.h: ltk_ul_gconv_f16): weight (n_sets, Cout, Cin, k, k), scale / shift
        (n_sets, Cout), sets[n] = image n's weight set; views = {x_ld, x_coff, y_ld, y_coff, res_ld, res_coff}.  -> the report as a dict."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        n_sets, Cout = int(w.shape[0]), int(w.shape[1])
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        st = np.ascontiguousarray(np.asarray(sets, dtype=np.int32))
        opts = _lib.ConvOpts()
        for key, v in (views or {}).items():
            setattr(opts, key, int(v))
        rep = _lib.ConvReport()
        _lib.check(self._lib.ltk_ul_gconv_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(H), int(W), int(Cin), w.ctypes.data, n_sets,
                                              st.ctypes.data, Cout, int(k), int(stride), int(pad), sc.ctypes.data if sc is not None else None,
                                              sf.ctypes.data if sf is not None else None, C.c_void_p(d_res_ptr) if d_res_ptr else None,
                                              int(bool(relu)), C.c_void_p(d_y_ptr), C.byref(opts), C.byref(rep)))
        return {"kernel": rep.kernel.decode(), "tile_px": rep.PXW, "tile_co": rep.NBT, "ksteps": rep.T, "blocks": rep.grid,
                "grid": (rep.items >> 16, rep.items & 0xFFFF, rep.NB)}

    @staticmethod
    def _ul_ir_report(rep) -> dict:
        return {"accepted": bool(rep.accepted), "reason": rep.reason.decode(), "kernel": rep.kernel.decode(), "Ho": rep.Ho, "Wo": rep.Wo,
                "tile": (rep.TH, rep.TW), "MC": rep.MC, "chunks": rep.chunks, "hidden_px": rep.hidden_px, "lds_bytes": rep.lds_bytes,
                "lds_limit": rep.lds_limit, "grid": (rep.grid_x, rep.grid_y, rep.grid_z), "blocks": rep.blocks, "threads": rep.threads}

    @staticmethod
    def ul_ir_plan(N, H, W, Cin, mid, Cout, stride=1, has_res=False, tap=False, views: Optional[dict] = None) -> dict:
        """What the fused inverted residual's planner decides (ltk_debug_ul_ir_plan; no GPU, no engine): accepted or refused with the
        reason as text, the instantiation's name, the tile, MC and chunk count, hidden pixels per tile, LDS bytes, grid and blocks."""
        opts = _lib.ConvOpts()
        for key, v in (views or {}).items():
            setattr(opts, key, int(v))
        rep = _lib.UlIrReport()
        _lib.check(_lib.load().ltk_debug_ul_ir_plan(int(N), int(H), int(W), int(Cin), int(mid), int(Cout), int(stride), int(bool(has_res)),
                                                    int(bool(tap)), C.byref(opts), C.byref(rep)))
        return Engine._ul_ir_report(rep)

    def ul_ir_f16(self, d_x_ptr: int, N, H, W, Cin, stride, w1: np.ndarray, wd: np.ndarray, w2: np.ndarray, affine1=(None, None),
                  affine_d=(None, None), affine2=(None, None), d_res_ptr: int = 0, d_y_ptr: int = 0, views: Optional[dict] = None,
                  d_e1_ptr: int = 0, d_e2_ptr: int = 0) -> dict:
        """One inverted residual in one launch (include/ltk.h: ltk_ul_ir_f16): w1 (mid, Cin), wd (mid, 3, 3), w2 (Cout, mid); affine* =
        (scale, shift) fp32 or None; views as ul_gconv_f16; d_e1_ptr / d_e2_ptr: the tap buffers.  -> the planner's report."""
        a1 = np.ascontiguousarray(w1, dtype=np.float32)
        ad = np.ascontiguousarray(wd, dtype=np.float32)
        a2 = np.ascontiguousarray(w2, dtype=np.float32)
        mid, Cout = int(a1.shape[0]), int(a2.shape[0])
        keep = [np.ascontiguousarray(v, dtype=np.float32) if v is not None else None for pair in (affine1, affine_d, affine2) for v in pair]
        ptr = lambda v: v.ctypes.data if v is not None else None
        opts = _lib.ConvOpts()
        for key, v in (views or {}).items():
            setattr(opts, key, int(v))
        rep = _lib.UlIrReport()
        _lib.check(self._lib.ltk_ul_ir_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(H), int(W), int(Cin), mid, Cout, int(stride),
                                           a1.ctypes.data, ad.ctypes.data, a2.ctypes.data, *[ptr(v) for v in keep],
                                           C.c_void_p(d_res_ptr) if d_res_ptr else None, C.c_void_p(d_y_ptr), C.byref(opts),
                                           C.c_void_p(d_e1_ptr) if d_e1_ptr else None, C.c_void_p(d_e2_ptr) if d_e2_ptr else None,
                                           C.byref(rep)))
        return Engine._ul_ir_report(rep)

    def ultralight_paste_back(self, avatar_id: int, idx: int, d_pred_ptr: int, out: np.ndarray, stream: int = 0):
        """out: C-contiguous uint8 (H,W,3) host array, filled in place (ultralight_avatar.py:173-184)."""
        _lib.check(self._lib.ltk_ultralight_paste_back(self._h, int(avatar_id), int(idx), C.c_void_p(d_pred_ptr), out.ctypes.data, 0,
                                                       C.c_void_p(stream)))

    def ultralight_paste_back_batch(self, avatar_id: int, idx: Sequence[int], d_pred_ptr: int, out_ptr: int, stream: int = 0):
        """n = len(idx) composites (n contiguous device uint8 [160][160][3] predictions) into host memory at out_ptr [n][H][W][3]
        (pinned for the PCIe rate): one device-to-host copy, one synchronisation (include/ltk.h: ltk_ultralight_paste_back_batch)."""
        arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int32))
        _lib.check(self._lib.ltk_ultralight_paste_back_batch(self._h, int(avatar_id), arr.ctypes.data, C.c_void_p(d_pred_ptr),
                                                             int(arr.size), C.c_void_p(out_ptr), C.c_void_p(stream)))

    def ultralight_forward_host(self, avatar_id: int, img6: np.ndarray, feat: np.ndarray) -> np.ndarray:
        """Model.forward on explicit inputs: img6 (B,6,160,160) in [0,1], feat (B,16,32,32) or (B,16,1024) -> sigmoid (B,3,160,160)."""
        img6 = np.ascontiguousarray(img6, dtype=np.float32)
        B = img6.shape[0]
        feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(B, 16, 32, 32)
        assert img6.shape[1:] == (6, 160, 160)
        pred = np.empty((B, 3, 160, 160), dtype=np.float32)
        _lib.check(self._lib.ltk_ultralight_forward_host(self._h, int(avatar_id), img6.ctypes.data, feat.ctypes.data, B, pred.ctypes.data))
        return pred

    def ultralight_ops(self, avatar_id: int):
        """[(tap name, type)] of the avatar's launch program in execution order; type 0 dense conv (as musetalk_ops()), 10 depthwise
        conv, 11 upsample, 12 input conv, 13 feature pack, 14 head, 15 a fused inverted residual (knob UL_FUSE_IR: listed once, under its
        project conv's name; the list follows the knob's current value)."""
        out = []
        buf = C.create_string_buffer(160)
        t = C.c_int()
        for i in range(self._lib.ltk_ultralight_op_count(self._h, int(avatar_id))):
            _lib.check(self._lib.ltk_ultralight_op_name(self._h, int(avatar_id), i, buf, 160, C.byref(t)))
            out.append((buf.value.decode(), t.value))
        return out

    def ultralight_time(self, avatar_id: int, frames: int, iters: int):
        ms = C.c_float()
        macs = C.c_double()
        _lib.check(self._lib.ltk_ultralight_time(self._h, int(avatar_id), int(frames), int(iters), C.byref(ms), C.byref(macs)))
        return ms.value, macs.value

    def dwconv3x3_f16(self, d_x_ptr: int, N, H, W, C_, weight: np.ndarray, stride: int = 1, scale=None, shift=None, relu: bool = True,
                      d_y_ptr: int = 0):
        """Depthwise 3x3 pad-1 conv on a CB16 tensor (include/ltk.h: ltk_dwconv3x3_f16); weight (C,1,3,3)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        _lib.check(self._lib.ltk_dwconv3x3_f16(self._h, C.c_void_p(d_x_ptr), N, H, W, C_, w.ctypes.data, int(stride),
                                               sc.ctypes.data if sc is not None else None, sf.ctypes.data if sf is not None else None,
                                               1 if relu else 0, C.c_void_p(d_y_ptr)))

    def upsample2x_cat_f16(self, d_x_ptr: int, N, h, w, C_up, d_skip_ptr: int, Hs, Ws, C_skip, d_y_ptr: int):
        """cat([bilinear x2 (align_corners) of x, skip]) on CB16 tensors (include/ltk.h: ltk_upsample2x_cat_f16)."""
        _lib.check(self._lib.ltk_upsample2x_cat_f16(self._h, C.c_void_p(d_x_ptr), N, h, w, C_up, C.c_void_p(d_skip_ptr), Hs, Ws, C_skip,
                                                    C.c_void_p(d_y_ptr)))

    # ---- the face parser's own ops (include/ltk.h: "Standalone ops of the BiSeNet face parser"); views = {x_ld, x_coff, y_ld, y_coff,
    # res_ld, res_coff} in channels
    def parse_stem_f16(self, d_rgb_ptr: int, N, H, W, weight: np.ndarray, scale=None, shift=None, d_y_ptr: int = 0,
                       views: Optional[dict] = None):
        """7x7 stride-2 stem + BatchNorm + ReLU on device uint8 RGB [N][H][W][3], normalisation fused; weight (64,3,7,7)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        assert w.shape == (64, 3, 7, 7)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_parse_stem_f16(self._h, C.c_void_p(d_rgb_ptr), int(N), int(H), int(W), w.ctypes.data,
                                                sc.ctypes.data if sc is not None else None, sf.ctypes.data if sf is not None else None,
                                                C.c_void_p(d_y_ptr), C.byref(o)))

    def maxpool3x3s2_f16(self, d_x_ptr: int, N, H, W, C_, d_y_ptr: int, views: Optional[dict] = None):
        """nn.MaxPool2d(3, 2, 1) on a CB16 tensor (padding -inf)."""
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_maxpool3x3s2_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(H), int(W), int(C_), C.c_void_p(d_y_ptr), C.byref(o)))

    def global_avgpool_f16(self, d_x_ptr: int, N, P, C_, d_y_ptr: int, views: Optional[dict] = None):
        """Mean over the P pixels of each channel of a CB16 tensor -> [N][C/16][1][16]."""
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_global_avgpool_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(P), int(C_), C.c_void_p(d_y_ptr), C.byref(o)))

    def chan_gate_f16(self, d_x_ptr: int, N, P, C_, d_a_ptr: int, d_y_ptr: int, d_b_ptr: int = 0, d_r_ptr: int = 0, plus1: bool = False,
                      views: Optional[dict] = None):
        """y = x * (sigmoid(a) [+ 1]) [+ b] [+ r] on CB16 tensors; a, b are [N][C/16][1][16]."""
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_chan_gate_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(P), int(C_), C.c_void_p(d_a_ptr),
                                               C.c_void_p(d_b_ptr) if d_b_ptr else None, C.c_void_p(d_r_ptr) if d_r_ptr else None,
                                               1 if plus1 else 0, C.c_void_p(d_y_ptr), C.byref(o)))

    def seg_argmax_f16(self, d_x_ptr: int, N, h, w, d_labels_ptr: int):
        """uint8 labels [N][8h][8w]: argmax over classes 0..18 of the bilinear x8 (align_corners) upsample of [N][2][h][w][16] logits."""
        _lib.check(self._lib.ltk_seg_argmax_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(h), int(w), C.c_void_p(d_labels_ptr)))

    @staticmethod
    def face_parse_program(size: int = 512):
        """The face parser's launch list at `size`, on the host alone (include/ltk.h: ltk_debug_face_parse_program): a dict per launch."""
        ops = (_lib.FpOpInfo * 64)()
        n = C.c_int()
        _lib.check(_lib.load().ltk_debug_face_parse_program(int(size), ops, 64, C.byref(n)))
        return [dict(name=o.name.decode(), **{f: getattr(o, f) for f, _ in _lib.FpOpInfo._fields_[1:]}) for o in ops[:n.value]]

    @staticmethod
    def face_parse_plan(size: int = 512, max_images: int = 1):
        """Where every launch of face_parse_program(size) reads and writes (include/ltk.h: ltk_debug_face_parse_plan), on the host
        alone: dict(ops=[dict(name, x, y, r, a, b)], buf_bytes=[...], image_buf, label_buf).  A view is dict(buf, ld, coff, C, H, W),
        or None where the op has no such operand."""
        ops = (_lib.FpBind * 64)()
        bufs = (C.c_ulonglong * 64)()
        n, nb, ib, lb = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.load().ltk_debug_face_parse_plan(int(size), int(max_images), ops, 64, C.byref(n), bufs, 64, C.byref(nb), C.byref(ib),
                                                         C.byref(lb)))

        def view(v):
            return None if v.buf < 0 else {f: int(getattr(v, f)) for f, _ in _lib.FpView._fields_}
        return dict(ops=[dict(name=o.name.decode(), **{k: view(getattr(o, k)) for k in ("x", "y", "r", "a", "b")}) for o in ops[:n.value]],
                    buf_bytes=[int(b) for b in bufs[:nb.value]], image_buf=ib.value, label_buf=lb.value)

    # ---- the face detector's own ops (include/ltk.h: "Standalone ops of the S3FD face detector"); views as above
    def s3fd_stem_f16(self, d_bgr_ptr: int, N, H, W, weight: np.ndarray, bias=None, d_y_ptr: int = 0, views: Optional[dict] = None):
        """conv1_1 + ReLU on device uint8 BGR [N][H][W][3], channel reversal and mean subtraction fused; weight (64,3,3,3)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        assert w.shape == (64, 3, 3, 3)
        b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        assert b is None or b.shape == (64,)
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_s3fd_stem_f16(self._h, C.c_void_p(d_bgr_ptr), int(N), int(H), int(W), w.ctypes.data,
                                               b.ctypes.data if b is not None else None, C.c_void_p(d_y_ptr), C.byref(o)))

    def maxpool2x2s2_f16(self, d_x_ptr: int, N, H, W, C_, d_y_ptr: int, views: Optional[dict] = None):
        """F.max_pool2d(x, 2, 2) on a CB16 tensor (floor mode)."""
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_maxpool2x2s2_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(H), int(W), int(C_), C.c_void_p(d_y_ptr), C.byref(o)))

    def l2norm_f16(self, d_x_ptr: int, N, P, C_, weight: np.ndarray, d_y_ptr: int, views: Optional[dict] = None):
        """L2Norm over the C channels of each of P pixels of a CB16 tensor; weight (C,)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        assert w.shape == (int(C_),)
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_l2norm_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(P), int(C_), w.ctypes.data, C.c_void_p(d_y_ptr), C.byref(o)))

    def s3fd_detect_f16(self, d_x_ptr: int, N, H, W, maxout: bool, level: int, thresh: float, d_recs_ptr: int, cap: int, d_counts_ptr: int,
                        views: Optional[dict] = None):
        """One level's candidates of a merged head map appended to recs [N][cap][6 words] through counts [N] (not reset here)."""
        o = _lib.ConvOpts(**{k: int(v) for k, v in (views or {}).items()})
        _lib.check(self._lib.ltk_s3fd_detect_f16(self._h, C.c_void_p(d_x_ptr), int(N), int(H), int(W), 1 if maxout else 0, int(level),
                                                 float(thresh), C.c_void_p(d_recs_ptr), int(cap), C.c_void_p(d_counts_ptr), C.byref(o)))

    @staticmethod
    def face_detect_program(H: int, W: int):
        """The face detector's launch list at H x W, on the host alone (include/ltk.h: ltk_debug_face_detect_program): a dict per launch."""
        ops = (_lib.FdOpInfo * 64)()
        n = C.c_int()
        _lib.check(_lib.load().ltk_debug_face_detect_program(int(H), int(W), ops, 64, C.byref(n)))
        return [dict(name=o.name.decode(), **{f: getattr(o, f) for f, _ in _lib.FdOpInfo._fields_[1:]}) for o in ops[:n.value]]

    @staticmethod
    def face_detect_plan(H: int, W: int, max_images: int = 16):
        """Where every launch of face_detect_program(H, W) reads and writes (include/ltk.h: ltk_debug_face_detect_plan), on the host
        alone: dict(ops=[dict(name, x, y)], buf_bytes=[...], image_buf, total_bytes).  A view is dict(buf, ld, coff, C, H, W), or None."""
        ops = (_lib.FdBind * 64)()
        bufs = (C.c_ulonglong * 64)()
        n, nb, ib, tot = C.c_int(), C.c_int(), C.c_int(), C.c_ulonglong()
        _lib.check(_lib.load().ltk_debug_face_detect_plan(int(H), int(W), int(max_images), ops, 64, C.byref(n), bufs, 64, C.byref(nb),
                                                          C.byref(ib), C.byref(tot)))

        def view(v):
            return None if v.buf < 0 else {f: int(getattr(v, f)) for f, _ in _lib.FpView._fields_}
        return dict(ops=[dict(name=o.name.decode(), x=view(o.x), y=view(o.y)) for o in ops[:n.value]],
                    buf_bytes=[int(b) for b in bufs[:nb.value]], image_buf=ib.value, total_bytes=int(tot.value))

    # ------------------------------------------------------------------ avatar preparation (face parser: blend-mask labels)
    def load_face_parser(self, sd: Dict[str, object], size: int = 512, max_images: int = 1):
        """face_parsing/__init__.py:44-56: `sd` = BiSeNet(n_classes=19).state_dict() (79999_iter.pth), tensors or arrays; the unused
        conv_out16 / conv_out32 heads may be present.  size: the square image size (the reference parses at 512); max_images: images
        per run of the program."""
        arr, n, keep = self._named_tensors(sd)
        _lib.check(self._lib.ltk_face_parse_load(self._h, arr, n, int(size), int(max_images)))
        self.face_parse_size = int(size)
        del keep

    def face_parse(self, rgb: np.ndarray) -> np.ndarray:
        """uint8 RGB (n, S, S, 3) at the loaded size -> uint8 labels (n, S, S), classes 0..18 (include/ltk.h: ltk_face_parse)."""
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[0] < 1 or rgb.shape[3] != 3 or rgb.shape[1] != rgb.shape[2]:
            raise ValueError(f"face_parse: uint8 (n, S, S, 3) expected, got {rgb.dtype} {rgb.shape}")
        size = self.face_parse_size
        if size is not None and rgb.shape[1] != size:
            raise ValueError(f"face_parse: the parser was loaded for {size} x {size} images, got {rgb.shape[1]} x {rgb.shape[2]}")
        rgb = np.ascontiguousarray(rgb)
        out = np.empty(rgb.shape[:3], dtype=np.uint8)
        # (before a load the library refuses with LTK_E_STATE)
        _lib.check(self._lib.ltk_face_parse(self._h, rgb.ctypes.data, int(rgb.shape[0]), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ avatar preparation (face detector: face boxes)
    def load_face_detector(self, sd: Dict[str, object], max_images: int = 16):
        """sfd_detector.py:26-29: `sd` = s3fd().state_dict() (s3fd.pth), tensors or arrays.  max_images: images per run of a program
        (the reference's face_det_batch_size)."""
        arr, n, keep = self._named_tensors(sd)
        _lib.check(self._lib.ltk_face_detect_load(self._h, arr, n, int(max_images)))
        del keep

    def face_detect(self, frames_bgr: np.ndarray, thresh: float = 0.05, cap: int = 4096, return_keys: bool = False):
        """uint8 BGR frames (n, H, W, 3) as cv2.imread gives them -> per image a float32 (k_i, 5) array of (x1, y1, x2, y2, score), the
        positions whose score is above `thresh`, in key order (level, row, column) (include/ltk.h: ltk_face_detect).  Raises when an
        image has more than `cap` candidates.  return_keys: also the uint32 keys, level << 28 | h << 14 | w."""
        f = np.ascontiguousarray(frames_bgr)
        if f.dtype != np.uint8 or f.ndim != 4 or f.shape[0] < 1 or f.shape[3] != 3:
            raise ValueError(f"face_detect: uint8 (n, H, W, 3) expected, got {f.dtype} {f.shape}")
        n = int(f.shape[0])
        cand = np.zeros((n, int(cap), 6), dtype=np.uint32)
        counts = np.zeros(n, dtype=np.int32)
        _lib.check(self._lib.ltk_face_detect(self._h, f.ctypes.data, n, int(f.shape[1]), int(f.shape[2]), float(thresh), cand.ctypes.data,
                                             int(cap), counts.ctypes.data))
        over = [i for i in range(n) if counts[i] > cap]
        if over:
            raise RuntimeError(f"face_detect: image {over[0]} has {int(counts[over[0]])} candidates above {thresh}, the lists hold {cap}")
        rows = [np.ascontiguousarray(cand[i, :counts[i], 1:]).view(np.float32) for i in range(n)]
        if return_keys:
            return rows, [cand[i, :counts[i], 0].copy() for i in range(n)]
        return rows

    def face_detect_debug_get(self, name: str, shape) -> np.ndarray:
        """The output of the launch `name` as the last run left it: float32 (images, cout, Ho, Wo); a merged head has 16 channels."""
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_face_detect_debug_get(self._h, name.encode(), int(shape[0]), out.ctypes.data, out.size))
        return out

    def face_detect_time(self, images: int, iters: int, per_op: bool = False):
        """(ms per device pass of `images` images of the last call's frame size as ltk_face_detect replays it, per-launch ms or None)."""
        ms = C.c_float()
        ops = (C.c_float * 39)() if per_op else None
        _lib.check(self._lib.ltk_debug_face_detect_time(self._h, int(images), int(iters), C.byref(ms), ops, 39 if per_op else 0))
        return ms.value, (list(ops) if per_op else None)

    def face_parse_debug_get(self, name: str, shape) -> np.ndarray:
        """The output of the launch `name` as the last run left it: float32 (images, cout, Ho, Wo), real channels only."""
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_face_parse_debug_get(self._h, name.encode(), int(shape[0]), out.ctypes.data, out.size))
        return out

    def face_parse_time(self, images: int, iters: int, per_op: bool = False):
        """(ms per device pass of `images` images as ltk_face_parse replays it, per-launch ms or None)."""
        ms = C.c_float()
        ops = (C.c_float * 41)() if per_op else None
        _lib.check(self._lib.ltk_debug_face_parse_time(self._h, int(images), int(iters), C.byref(ms), ops, 41 if per_op else 0))
        return ms.value, (np.array(ops[:], dtype=np.float64) if per_op else None)

    # ---- frame egress (include/ltk.h: ltk_egress_*)
    def egress_open(self, H: int, W: int) -> int:
        h = C.c_void_p()
        _lib.check(self._lib.ltk_egress_open(self._h, int(H), int(W), C.byref(h)))
        with self._lock:
            self._egress_open.add(h.value)
        return h.value

    def egress_close(self, session: int) -> None:
        """No-op on a session this engine no longer holds (closed already, or closed with the engine)."""
        with self._lock:
            if not self._h or session not in self._egress_open:
                return
            self._egress_open.discard(session)
        _lib.check(self._lib.ltk_egress_close(self._h, C.c_void_p(session)))

    def egress_watermark(self, session: int, mask, x: int = 0, y: int = 0, color=(128, 128, 128)) -> None:
        if mask is None:
            _lib.check(self._lib.ltk_egress_watermark(self._h, C.c_void_p(session), None, 0, 0, 0, 0, 0, 0, 0))
            return
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        _lib.check(self._lib.ltk_egress_watermark(self._h, C.c_void_p(session), mask.ctypes.data, int(x), int(y), mask.shape[1],
                                                  mask.shape[0], int(color[0]), int(color[1]), int(color[2])))

    def egress_frame(self, session: int, out: np.ndarray, source: int, avatar_id: int = 0, idx: int = 0, d_pred_ptr: int = 0,
                     h_frame: np.ndarray = None, speaking: bool = True, alpha: float = -1.0, keep: bool = False, fmt: int = 0,
                     chroma: int = 1, stream: int = 0) -> np.ndarray:
        req = _lib.EgressReq(int(source), int(avatar_id), int(idx), C.c_void_p(d_pred_ptr or None),
                             C.c_void_p(h_frame.ctypes.data if h_frame is not None else None), int(bool(speaking)), float(alpha),
                             int(bool(keep)), int(fmt), int(chroma))
        _lib.check(self._lib.ltk_egress_frame(self._h, C.c_void_p(session), C.byref(req), out.ctypes.data, C.c_void_p(stream)))
        return out

    def egress_batch(self, session: int, source: int, avatar_id: int, idx: Sequence[int], d_pred_ptr: int, out_ptr: int, fmt: int = 0,
                     chroma: int = 1, stream: int = 0) -> None:
        """The speaking frames of one inference_batch result: len(idx) composites + watermark + format conversion on the device, one
        device-to-host copy into host memory at out_ptr (include/ltk.h: ltk_egress_batch)."""
        arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int32))
        _lib.check(self._lib.ltk_egress_batch(self._h, C.c_void_p(session), int(source), int(avatar_id), arr.ctypes.data,
                                              C.c_void_p(d_pred_ptr), int(arr.size), int(fmt), int(chroma), C.c_void_p(out_ptr),
                                              C.c_void_p(stream)))

    def musetalk_forward_host(self, latents: np.ndarray, feat: np.ndarray, want_image=True, want_frames=True):
        latents = np.ascontiguousarray(latents, dtype=np.float32).reshape(-1, 8, 32, 32)
        feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1, 50, 384)
        B = latents.shape[0]
        unet_out = np.empty((B, 4, 32, 32), dtype=np.float32)
        image = np.empty((B, 3, 256, 256), dtype=np.float32) if want_image else None
        frames = np.empty((B, 256, 256, 3), dtype=np.uint8) if want_frames else None
        _lib.check(self._lib.ltk_musetalk_forward_host(self._h, latents.ctypes.data, feat.ctypes.data, B, unet_out.ctypes.data,
                                                       image.ctypes.data if want_image else None,
                                                       frames.ctypes.data if want_frames else None))
        return unet_out, image, frames

    def musetalk_debug_get_q8(self, op: str, shape) -> np.ndarray:
        """Raw e4m3 codes (uint8, shape (frames, C, H * W)) of an fp8-path op's output as the last pass left it (include/ltk.h)."""
        out = np.empty(shape, dtype=np.uint8)
        _lib.check(self._lib.ltk_musetalk_debug_get_q8(self._h, op.encode(), int(shape[0]), out.ctypes.data, out.size))
        return out

    def musetalk_debug_get(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_musetalk_debug_get(self._h, name.encode(), int(shape[0]), out.ctypes.data, out.size))
        return out

    def musetalk_info(self):
        macs, macs8 = C.c_double(), C.c_double()
        _lib.check(self._lib.ltk_musetalk_info(self._h, C.byref(macs), C.byref(macs8)))
        return macs.value, macs8.value

    def musetalk_ops(self):
        """[(name, type)] of the MuseTalk launch program; type 0 conv/linear, 1 GroupNorm, 2 LayerNorm, 3 attention, 4 GEGLU, 5 add-pos, 6 value transpose."""
        out = []
        for i in range(self._lib.ltk_musetalk_op_count(self._h)):
            buf, t = C.create_string_buffer(160), C.c_int()
            _lib.check(self._lib.ltk_musetalk_op_name(self._h, i, buf, 160, C.byref(t)))
            out.append((buf.value.decode(), t.value))
        return out

    def musetalk_time_ops(self, frames: int, iters: int) -> np.ndarray:
        n = self._lib.ltk_musetalk_op_count(self._h)
        ms = (C.c_float * n)()
        _lib.check(self._lib.ltk_musetalk_time_ops(self._h, int(frames), int(iters), ms, n))
        return np.array(ms[:], dtype=np.float64)

    def musetalk_time(self, frames: int, iters: int):
        ms = C.c_float()
        macs = C.c_double()
        _lib.check(self._lib.ltk_musetalk_time(self._h, int(frames), int(iters), C.byref(ms), C.byref(macs)))
        return ms.value, macs.value

    # ------------------------------------------------------------------ avatar preparation (VAE encoder)
    def load_vae_encoder(self, vae_sd: Dict[str, object], max_faces: int = 8):
        sd = {k: v for k, v in vae_sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}
        arr, n, keep = self._named_tensors(sd)
        _lib.check(self._lib.ltk_vae_encoder_load(self._h, arr, n, int(max_faces)))
        del keep

    def vae_encode_faces(self, faces_bgr: np.ndarray, noise: Optional[np.ndarray] = None) -> np.ndarray:
        """vae.get_latents_for_unet for each 256x256 BGR crop -> fp32 (n, 8, 32, 32)."""
        faces = np.ascontiguousarray(faces_bgr, dtype=np.uint8).reshape(-1, 256, 256, 3)
        n = faces.shape[0]
        out = np.empty((n, 8, 32, 32), dtype=np.float32)
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).reshape(n, 2, 4, 32, 32)
        _lib.check(self._lib.ltk_vae_encode_faces(self._h, faces.ctypes.data, n, nz.ctypes.data if nz is not None else None,
                                                  out.ctypes.data))
        return out

    # ------------------------------------------------------------------ whisper audio features
    def load_whisper(self, encoder_sd: Dict[str, object]):
        """audio2feature.py:15-23: `encoder_sd` = WhisperModel.from_pretrained(...).encoder.state_dict()."""
        arr, n, keep = self._named_tensors(encoder_sd)
        _lib.check(self._lib.ltk_whisper_load(self._h, arr, n))
        del keep

    def whisper_step(self, pcm: np.ndarray, batch: int, first_row: int, d_out_ptr: int, row_step: int = 2, rows: int = 10,
                     stream: int = 0):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        _lib.check(self._lib.ltk_whisper_step(self._h, pcm.ctypes.data, pcm.shape[0], int(batch), int(first_row), int(row_step),
                                              int(rows), C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def whisper_debug_get(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_whisper_debug_get(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def whisper_step_batch(self, reqs: Sequence[tuple]):
        """The live steps of several MuseTalk sessions in one call: reqs = [(pcm, batch, first_row, row_step, rows, d_out_ptr)].  Up to
        16 clips share one run of the batched encoder program (ltk_whisper_step_batch); one request is whisper_step."""
        arr = (WhisperReq * len(reqs))()
        keep = []                                      # the pcm arrays stay alive across the call
        for i, (pcm, batch, first_row, row_step, rows, d_out_ptr) in enumerate(reqs):
            pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
            keep.append(pcm)
            arr[i].pcm, arr[i].n_samples = pcm.ctypes.data, pcm.shape[0]
            arr[i].batch, arr[i].first_row, arr[i].row_step, arr[i].rows = int(batch), int(first_row), int(row_step), int(rows)
            arr[i].d_out = d_out_ptr
        _lib.check(self._lib.ltk_whisper_step_batch(self._h, arr, len(reqs)))
        del keep

    def whisper_batch_info(self) -> dict:
        """capacity: clips per batched run; built: 1 once the batched program exists (the first batched run builds it);
        activation_bytes: its activations at full capacity (0 until built)."""
        cap, built, act = C.c_int(), C.c_int(), C.c_size_t()
        _lib.check(self._lib.ltk_whisper_batch_info(self._h, C.byref(cap), C.byref(built), C.byref(act)))
        return {"capacity": cap.value, "built": built.value, "activation_bytes": int(act.value)}

    def whisper_debug_get_clip(self, name: str, clip: int, shape) -> np.ndarray:
        """A named tensor (the names whisper_debug_get takes) of clip `clip` of the batched run that ran last."""
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_whisper_debug_get_clip(self._h, name.encode(), int(clip), out.ctypes.data, out.size))
        return out

    def whisper_batch_plan(self, nreq: int):
        """How whisper_step_batch cuts a call of nreq requests (host only): [(batched, [requests in slot order])] in execution order."""
        n = max(int(nreq), 1)
        run_of, slot_of, batched, n_runs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), C.c_int()
        _lib.check(self._lib.ltk_debug_whisper_batch_plan(int(nreq), run_of, slot_of, batched, C.byref(n_runs)))
        runs = [(bool(batched[i]), []) for i in range(n_runs.value)]
        for r in sorted(range(int(nreq)), key=lambda r: (run_of[r], slot_of[r])):
            runs[run_of[r]][1].append(r)
        return runs

    # ------------------------------------------------------------------ hubert audio features (Ultralight)
    @staticmethod
    def fold_hubert_weight_norm(state_dict: Dict[str, object]) -> Dict[str, np.ndarray]:
        """HubertModel.state_dict() -> the names ltk_hubert_load takes: the positional conv's weight norm folded into
        "encoder.pos_conv_embed.conv.weight" = g * v / ||v||, the norm over dims (0, 1) for every tap (weight_norm(conv, dim=2)).
        Both spellings are accepted: parametrizations.weight.original0 / original1 and weight_g / weight_v; a state dict that already
        has the folded weight passes through."""
        p = "encoder.pos_conv_embed.conv."
        pairs = ((p + "parametrizations.weight.original0", p + "parametrizations.weight.original1"), (p + "weight_g", p + "weight_v"))
        sd = {k: v for k, v in state_dict.items() if k != "masked_spec_embed"}
        for gk, vk in pairs:
            if gk in sd and vk in sd:
                g = _as_f32(sd.pop(gk)).astype(np.float64)
                v = _as_f32(sd.pop(vk)).astype(np.float64)
                norm = np.sqrt((v * v).sum(axis=(0, 1), keepdims=True))
                sd[p + "weight"] = (g.reshape(1, 1, -1) * v / norm).astype(np.float32)
        if p + "weight" not in sd:
            raise KeyError("state_dict has neither the positional conv's weight-norm pair (either spelling) nor its folded weight")
        return sd

    def load_hubert(self, state_dict: Dict[str, object]):
        """avatars/ultralight/audio2feature.py:9-11: `state_dict` = HubertModel.from_pretrained(...).state_dict()."""
        arr, n, keep = self._named_tensors(self.fold_hubert_weight_norm(state_dict))
        _lib.check(self._lib.ltk_hubert_load(self._h, arr, n))
        del keep

    def hubert_features(self, pcm: np.ndarray) -> np.ndarray:
        """get_hubert_from_16k_speech: 16 kHz float pcm -> float32 ((n - 80) // 320, 1024) on the host."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        expected = max((pcm.shape[0] - 80) // 320, 1)
        out = np.empty((expected, 1024), dtype=np.float32)
        rows = C.c_int()
        _lib.check(self._lib.ltk_hubert_features(self._h, pcm.ctypes.data, pcm.shape[0], out.ctypes.data, expected, C.byref(rows)))
        return out[: rows.value]

    def hubert_step(self, pcm: np.ndarray, batch: int, first_row: int, d_out_ptr: int, row_step: int = 2, rows: int = 16):
        """One forward of the step's pcm and the chunk gather into device float32 [batch][rows][1024] at d_out_ptr."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        _lib.check(self._lib.ltk_hubert_step(self._h, pcm.ctypes.data, pcm.shape[0], int(batch), int(first_row), int(row_step), int(rows),
                                             C.c_void_p(d_out_ptr)))

    def hubert_step_batch(self, reqs: Sequence[tuple]):
        """The live steps of several sessions in one call: reqs = [(pcm, batch, first_row, row_step, rows, d_out_ptr)].  Clips of one
        length share a program run of up to 16 (ltk_hubert_step_batch); one request is hubert_step."""
        arr = (HubertReq * len(reqs))()
        keep = []                                      # the pcm arrays stay alive across the call
        for i, (pcm, batch, first_row, row_step, rows, d_out_ptr) in enumerate(reqs):
            pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
            keep.append(pcm)
            arr[i].pcm, arr[i].n_samples = pcm.ctypes.data, pcm.shape[0]
            arr[i].batch, arr[i].first_row, arr[i].row_step, arr[i].rows = int(batch), int(first_row), int(row_step), int(rows)
            arr[i].d_out = d_out_ptr
        _lib.check(self._lib.ltk_hubert_step_batch(self._h, arr, len(reqs)))
        del keep

    def hubert_debug_get_clip(self, name: str, clip: int, shape) -> np.ndarray:
        """A named tensor (or "input_values") of clip `clip` of the batched run that ran last."""
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_debug_get_clip(self._h, name.encode(), int(clip), out.ctypes.data, out.size))
        return out

    def hubert_batch_info(self) -> dict:
        cap, progs, act = C.c_int(), C.c_int(), C.c_size_t()
        _lib.check(self._lib.ltk_hubert_batch_info(self._h, C.byref(cap), C.byref(progs), C.byref(act)))
        return {"capacity": cap.value, "programs": progs.value, "activation_bytes": act.value}

    def hubert_debug_get(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_debug_get(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def hubert_ops(self):
        """[(name, type)] of a HuBERT program; type as musetalk_ops(), and 7 conv layer 0 + LayerNorm + GELU, 8 LayerNorm + GELU,
        9 positional conv."""
        out = []
        for i in range(self._lib.ltk_hubert_op_count(self._h)):
            buf, t = C.create_string_buffer(160), C.c_int()
            _lib.check(self._lib.ltk_hubert_op_name(self._h, i, buf, 160, C.byref(t)))
            out.append((buf.value.decode(), t.value))
        return out

    def hubert_info(self) -> dict:
        layers, progs, act = C.c_int(), C.c_int(), C.c_size_t()
        _lib.check(self._lib.ltk_hubert_info(self._h, C.byref(layers), C.byref(progs), C.byref(act)))
        return {"layers": layers.value, "programs": progs.value, "activation_bytes": int(act.value)}

    # the HuBERT kernels on their own (include/ltk.h: unit-test hooks); token-major in, token-major out
    def hubert_stats(self, pcm: np.ndarray):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        out = np.empty(2, dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_stats(self._h, pcm.ctypes.data, pcm.shape[0], out.ctypes.data))
        return float(out[0]), float(out[1])

    def hubert_layer0(self, x, w, bias, gamma, beta) -> np.ndarray:
        x, w, bias, gamma, beta = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, bias, gamma, beta))
        assert w.size == 5120 and bias.size == gamma.size == beta.size == 512
        out = np.empty((512, (x.size - 10) // 5 + 1), dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_layer0_host(self._h, x.ctypes.data, x.size, w.ctypes.data, bias.ctypes.data, gamma.ctypes.data,
                                                    beta.ctypes.data, out.ctypes.data))
        return np.ascontiguousarray(out.T)

    def hubert_ln_gelu(self, x, gamma, beta) -> np.ndarray:
        x, gamma, beta = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, gamma, beta))
        assert x.ndim == 2 and x.shape[1] == 512
        out = np.empty((512, x.shape[0]), dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_ln_gelu_host(self._h, x.ctypes.data, x.shape[0], gamma.ctypes.data, beta.ctypes.data, out.ctypes.data))
        return np.ascontiguousarray(out.T)

    def hubert_posconv(self, x, w, bias) -> np.ndarray:
        x, w, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, bias))
        assert x.ndim == 2 and x.shape[1] == 1024 and w.shape == (1024, 64, 128) and bias.size == 1024
        out = np.empty((1024, x.shape[0]), dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_posconv_host(self._h, x.ctypes.data, x.shape[0], w.ctypes.data, bias.ctypes.data, out.ctypes.data))
        return np.ascontiguousarray(out.T)

    def hubert_chunks(self, feat, batch: int, first_row: int, row_step: int = 2, rows: int = 16) -> np.ndarray:
        feat = np.ascontiguousarray(feat, dtype=np.float32)
        assert feat.ndim == 2 and feat.shape[1] == 1024
        out = np.empty((batch, rows, 1024), dtype=np.float32)
        _lib.check(self._lib.ltk_hubert_chunks_host(self._h, feat.ctypes.data, feat.shape[0], int(batch), int(first_row), int(row_step),
                                                    int(rows), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ fp16 headroom watch (include/ltk.h: ltk_health_*)
    @staticmethod
    def _health_program(program) -> int:
        if isinstance(program, str):
            if program not in _lib.HEALTH_PROGRAMS:
                raise ValueError(f"unknown program {program!r}: one of {sorted(_lib.HEALTH_PROGRAMS)}")
            return _lib.HEALTH_PROGRAMS[program]
        return int(program)

    @staticmethod
    def _health_dict(o) -> dict:
        return {"name": o.name.decode(), "type": int(o.type), "observed": int(o.observed), "q8": int(o.q8), "elements": int(o.elements),
                "at_limit": int(o.at_limit), "near_limit": int(o.near_limit), "nonfinite": int(o.nonfinite), "max_abs": float(o.max_abs),
                "limit": float(o.limit)}

    def health_watch(self, program, calls: int, avatar_id: int = -1):
        """Arm the next `calls` inference calls of `program` ("wav2lip", "musetalk", "ultralight", "whisper", "hubert", "faceparse" or an
        LTK_HEALTH_* code): each runs its usual launches with a scan behind every op.  0 disarms.  avatar_id: Ultralight only."""
        _lib.check(self._lib.ltk_health_watch(self._h, self._health_program(program), int(avatar_id), int(calls)))

    def health_report(self, program, avatar_id: int = -1):
        """(ops, calls_seen, calls_left): one dict per op of the program's listing (name, type, observed, q8, elements, at_limit,
        near_limit, nonfinite, max_abs, limit), accumulated over the watched calls since the watch was armed.  Waits for the device."""
        prog = self._health_program(program)
        cap = 1024
        ops = (_lib.HealthOp * cap)()
        n, seen, left = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.ltk_health_report(self._h, prog, int(avatar_id), ops, cap, C.byref(n), C.byref(seen), C.byref(left)))
        return [self._health_dict(ops[i]) for i in range(n.value)], int(seen.value), int(left.value)

    def health_scan(self, d_x: int, N: int, cbt: int, cb0: int, CB: int, P: int, q8: bool = False) -> dict:
        """The scan kernel on one tensor view: device fp16 [N][cbt][P][16] (or e4m3 [N][cbt][P][32] with q8), channel blocks
        [cb0, cb0 + CB).  The caller's work on d_x must be complete."""
        rec = _lib.HealthOp()
        _lib.check(self._lib.ltk_health_scan(self._h, int(d_x), int(N), int(cbt), int(cb0), int(CB), int(P), 1 if q8 else 0, C.byref(rec)))
        return self._health_dict(rec)

    # ------------------------------------------------------------------ test / measurement hooks
    def wav2lip_forward_host(self, mel: np.ndarray, face6: np.ndarray) -> np.ndarray:
        mel = np.ascontiguousarray(mel, dtype=np.float32).reshape(-1, 80, 16)
        face6 = np.ascontiguousarray(face6, dtype=np.float32)
        B = face6.shape[0]
        assert face6.shape[1:] == (6, 256, 256) and mel.shape[0] == B
        pred = np.empty((B, 3, 256, 256), dtype=np.float32)
        _lib.check(self._lib.ltk_wav2lip_forward_host(self._h, mel.ctypes.data, face6.ctypes.data, B, pred.ctypes.data))
        return pred

    @staticmethod
    def set_knob(name: str, value: int):
        """Process-wide tuning knob (csrc/tune.h); sweeps and A/B tests only."""
        lib = _lib.load()
        _lib.check(lib.ltk_debug_set_knob(name.encode(), int(value)))

    def debug_capture(self, enable: bool):
        _lib.check(self._lib.ltk_debug_capture(self._h, 1 if enable else 0))

    def debug_get(self, layer: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._lib.ltk_debug_get(self._h, layer.encode(), out.ctypes.data, out.size))
        return out

    def layer_names(self):
        n = self._lib.ltk_wav2lip_layer_count(self._h)
        out = []
        for i in range(n):
            buf = C.create_string_buffer(96)
            _lib.check(self._lib.ltk_wav2lip_layer_name(self._h, i, buf, 96))
            out.append(buf.value.decode())
        return out

    def set_layer_tile(self, layer: int, bucket: int, pxw: int = 0, nbt: int = 0, ksplit: int = 0):
        _lib.check(self._lib.ltk_wav2lip_set_layer_tile(self._h, int(layer), int(bucket), int(pxw), int(nbt), int(ksplit)))

    def time_layers(self, frames: int, iters: int) -> np.ndarray:
        n = self._lib.ltk_wav2lip_layer_count(self._h)
        ms = (C.c_float * n)()
        _lib.check(self._lib.ltk_wav2lip_time_layers(self._h, int(frames), int(iters), ms, n))
        return np.array(ms[:], dtype=np.float64)

    def graph_count(self) -> int:
        """Frame counts whose Wav2Lip pass currently replays from a captured hipGraph (include/ltk.h)."""
        return int(self._lib.ltk_wav2lip_graph_count(self._h))

    def face_cache_bytes(self, avatar_id: int) -> int:
        """Bytes of face-encoder skip cache the avatar holds (knob FACE_CACHE, include/ltk.h); 0 = none built."""
        n = C.c_size_t(0)
        _lib.check(self._lib.ltk_avatar_face_cache_bytes(self._h, int(avatar_id), C.byref(n)))
        return int(n.value)

    def prefetch_stats(self) -> dict:
        """Knob PREFETCH (include/ltk.h): single-request calls that found their face-encoder outputs prefetched by the previous
        call / that did not / prefetches issued."""
        h, m, i = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        _lib.check(self._lib.ltk_wav2lip_prefetch_stats(self._h, C.byref(h), C.byref(m), C.byref(i)))
        return {"hits": int(h.value), "misses": int(m.value), "issued": int(i.value)}

    def program_graph_count(self) -> int:
        """(program, frame count) pairs of the MuseTalk side (U-Net + VAE pass, Whisper encoder) that replay from a captured hipGraph."""
        return int(self._lib.ltk_program_graph_count(self._h))

    def time_convs(self, frames: int, iters: int):
        ms = C.c_float()
        macs = C.c_double()
        _lib.check(self._lib.ltk_wav2lip_time_convs(self._h, int(frames), int(iters), C.byref(ms), C.byref(macs)))
        return ms.value, macs.value

    def conv2d_fp8(self, d_x_ptr: int, N, H, W, Cin, weight: np.ndarray, Cout, scale=None, shift=None, act_scale: float = 8.0,
                   d_res_ptr: int = 0, act: int = 0, d_y_ptr: int = 0, iters: int = 0) -> float:
        """3x3 s1 p1 conv on e4m3 operands (include/ltk.h: ltk_conv2d_fp8); x is [N][Cin/32][H][W][32] bytes."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        ms = C.c_float(0)
        _lib.check(self._lib.ltk_conv2d_fp8(
            self._h, C.c_void_p(d_x_ptr), N, H, W, Cin, w.ctypes.data, Cout, sc.ctypes.data if sc is not None else None,
            sf.ctypes.data if sf is not None else None, float(act_scale), C.c_void_p(d_res_ptr) if d_res_ptr else None, int(act),
            C.c_void_p(d_y_ptr), iters, C.byref(ms)))
        return ms.value

    def groupnorm_f16(self, d_x_ptr: int, N, C_, P, groups, eps, gamma: np.ndarray, beta: np.ndarray, silu: bool, d_y_ptr: int, impl: int = 0,
                      out_fp8: bool = False, out_scale: float = 1.0, iters: int = 0) -> float:
        """Standalone GroupNorm(+SiLU) on a CB16 tensor (include/ltk.h: ltk_groupnorm_f16); impl 0 = the program's choice, 1 = two-pass,
        2 = one block per (image, group), 3 = one tensor pass with the exchange between blocks.  Returns ms per run when iters > 0."""
        ga = np.ascontiguousarray(gamma, dtype=np.float32)
        be = np.ascontiguousarray(beta, dtype=np.float32)
        ms = C.c_float(0)
        _lib.check(self._lib.ltk_groupnorm_f16(self._h, C.c_void_p(d_x_ptr), N, C_, P, groups, float(eps), ga.ctypes.data, be.ctypes.data,
                                               1 if silu else 0, impl, 1 if out_fp8 else 0, float(out_scale), C.c_void_p(d_y_ptr), iters, C.byref(ms)))
        return ms.value

    def groupnorm_f16_ex(self, d_x_ptr: int, N, C_, P, groups, eps, gamma: np.ndarray, beta: np.ndarray, silu: bool, d_y_ptr: int, impl: int = 0,
                         out_fp8: bool = False, out_scale: float = 1.0, **opts) -> dict:
        """GroupNorm(+SiLU) on channel views with a report of what ran (include/ltk.h: ltk_groupnorm_f16_ex; `opts` = the fields of
        ltk_norm_opts: x_ld, x_coff, y_ld, y_coff).  Returns the report as a dict (kernel: str, impl, segs, members, grid)."""
        ga = np.ascontiguousarray(gamma, dtype=np.float32)
        be = np.ascontiguousarray(beta, dtype=np.float32)
        o = _lib.NormOpts(**{name: int(v) for name, v in opts.items()})
        rep = _lib.NormReport()
        _lib.check(self._lib.ltk_groupnorm_f16_ex(self._h, C.c_void_p(d_x_ptr), N, C_, P, groups, float(eps), ga.ctypes.data, be.ctypes.data,
                                                  1 if silu else 0, impl, 1 if out_fp8 else 0, float(out_scale), C.c_void_p(d_y_ptr), C.byref(o),
                                                  C.byref(rep)))
        out = {name: getattr(rep, name) for name, _ in _lib.NormReport._fields_}
        out["kernel"] = rep.kernel.decode()
        return out

    POINTWISE_OPS = ("layernorm", "geglu", "gelu", "silu", "add_pos", "nchw_to_cb16", "tokens_to_cb16", "vae_post")

    def pointwise_f16(self, op: str, d_x_ptr: int, d_y_ptr: int, N, C_, P, eps: float = 0.0, v0: Optional[np.ndarray] = None,
                      v1: Optional[np.ndarray] = None, **opts) -> None:
        """One pointwise / layout kernel of csrc/nn_kernels.hip on its own (include/ltk.h: ltk_pointwise_f16); op: a name of
        POINTWISE_OPS, v0 / v1: gamma / beta of the LayerNorm, the position or additive table; `opts` = the fields of ltk_norm_opts."""
        a0 = np.ascontiguousarray(v0, dtype=np.float32) if v0 is not None else None
        a1 = np.ascontiguousarray(v1, dtype=np.float32) if v1 is not None else None
        o = _lib.NormOpts(**{name: int(v) for name, v in opts.items()})
        _lib.check(self._lib.ltk_pointwise_f16(self._h, self.POINTWISE_OPS.index(op), C.c_void_p(d_x_ptr) if d_x_ptr else None, C.c_void_p(d_y_ptr),
                                               N, C_, P, float(eps), a0.ctypes.data if a0 is not None else None,
                                               a1.ctypes.data if a1 is not None else None, C.byref(o)))

    def attention_f16(self, q, k, v, o, N, heads, d16, Tq, Tk, impl: int = 0) -> None:
        """Standalone attention on CB16 tensors (include/ltk.h: ltk_attention_f16).  q, k, v, o: (device pointer, cbt, cb0) each - the
        buffer, its channel blocks and the first block of head 0; impl 0 = the program's choice, 1 = the per-wave / wide kernel, 2 = the
        LDS form.  The 1 / sqrt(d) scale is the caller's."""
        args = []
        for ptr, cbt, cb0 in (q, k, v, o):
            args += [C.c_void_p(ptr), int(cbt), int(cb0)]
        _lib.check(self._lib.ltk_attention_f16(self._h, *args, N, heads, d16, Tq, Tk, impl))

    def conv2d_f16(self, d_x_ptr: int, N, H, W, Cin, weight: np.ndarray, Cout, k, stride, pad, transposed=False,
                   out_pad=0, scale: Optional[np.ndarray] = None, shift: Optional[np.ndarray] = None,
                   d_res_ptr: int = 0, relu=True, d_y_ptr: int = 0, iters: int = 0) -> float:
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        ms = C.c_float(0)
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        _lib.check(self._lib.ltk_conv2d_f16(
            self._h, C.c_void_p(d_x_ptr), N, H, W, Cin, w.ctypes.data, Cout, kh, kw, sh, sw, ph, pw,
            1 if transposed else 0, out_pad, sc.ctypes.data if sc is not None else None,
            sf.ctypes.data if sf is not None else None, C.c_void_p(d_res_ptr) if d_res_ptr else None,
            1 if relu else 0, C.c_void_p(d_y_ptr), iters, C.byref(ms)))
        return ms.value

    def conv2d_f16_ex(self, d_x_ptr: int, N, H, W, Cin, weight: np.ndarray, Cout, k, stride, pad, transposed=False, out_pad=0,
                      scale: Optional[np.ndarray] = None, shift: Optional[np.ndarray] = None, d_res_ptr: int = 0, d_y_ptr: int = 0,
                      **opts) -> dict:
        """One conv layer with the caller naming what runs (include/ltk.h: ltk_conv2d_f16_ex; `opts` = the fields of ltk_conv_opts:
        x_ld, x_coff, y_ld, y_coff, res_ld, res_coff, act, ups, force_pxw, force_nbt, force_ksplit, family).  Returns the report of
        what was launched as a dict (kernel: str, family, G, NBT, PXW, NC8, T, S, ksplit, items, grid, FT, UB)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        o = _lib.ConvOpts(**{name: int(v) for name, v in opts.items()})
        rep = _lib.ConvReport()
        _lib.check(self._lib.ltk_conv2d_f16_ex(
            self._h, C.c_void_p(d_x_ptr), N, H, W, Cin, w.ctypes.data, Cout, kh, kw, sh, sw, ph, pw, 1 if transposed else 0, out_pad,
            sc.ctypes.data if sc is not None else None, sf.ctypes.data if sf is not None else None,
            C.c_void_p(d_res_ptr) if d_res_ptr else None, 0, C.c_void_p(d_y_ptr), C.byref(o), C.byref(rep)))
        return _conv_report_dict(rep)

    @staticmethod
    def conv_plan(N, H, W, Cin, Cout, k, stride, pad, transposed=False, out_pad=0, has_res=False, **opts) -> dict:
        """What conv2d_f16_ex would report for this call, decided on the host alone (ltk_debug_conv_plan; no GPU needed): the same
        refusals (LtkError) up to the point where a launch would be enqueued, the same report dict."""
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        o = _lib.ConvOpts(**{name: int(v) for name, v in opts.items()})
        rep = _lib.ConvReport()
        _lib.check(_lib.load().ltk_debug_conv_plan(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, 1 if transposed else 0, out_pad,
                                                   1 if has_res else 0, 0, C.byref(o), C.byref(rep)))
        return _conv_report_dict(rep)

    @staticmethod
    def conv3_variants() -> list:
        """Names of every fp16 conv3 instantiation the launch path can pick (ltk_debug_conv3_variants); no GPU needed."""
        buf = C.create_string_buffer(8192)
        _lib.check(_lib.load().ltk_debug_conv3_variants(buf, len(buf)))
        return buf.value.decode().split()

    @staticmethod
    def conv1_variants() -> list:
        """Names of every instantiation of the first-generation kernel its picker can return (ltk_debug_conv1_variants); no GPU needed."""
        buf = C.create_string_buffer(8192)
        _lib.check(_lib.load().ltk_debug_conv1_variants(buf, len(buf)))
        return buf.value.decode().split()

    W2L_HEAD_OPS = ("conv7_bank", "conv7_packed", "audio0", "audio3", "convs2d")

    def w2l_head_f16(self, op: str, weight: np.ndarray, scale: np.ndarray, shift: np.ndarray, d_y_ptr: int, N: int, frame_ptrs=None,
                     d_x_ptr: int = 0, H: int = 0, W: int = 0, Cin: int = 0, Cout: int = 0, **opts) -> None:
        """One special-case kernel of csrc/conv7_mfma.hip on its own (include/ltk.h: ltk_w2l_head_f16); op: a name of W2L_HEAD_OPS;
        frame_ptrs: N device pointers of the per-frame inputs (conv7_bank, audio0), d_x_ptr: the other ops' input; `opts` = the fields of
        ltk_norm_opts."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32)
        sf = np.ascontiguousarray(shift, dtype=np.float32)
        o = _lib.NormOpts(**{name: int(v) for name, v in opts.items()})
        tab = (C.c_void_p * len(frame_ptrs))(*[int(p) for p in frame_ptrs]) if frame_ptrs is not None else None
        _lib.check(self._lib.ltk_w2l_head_f16(self._h, self.W2L_HEAD_OPS.index(op), tab, C.c_void_p(d_x_ptr) if d_x_ptr else None, N, H, W, Cin, Cout,
                                              w.ctypes.data, sc.ctypes.data, sf.ctypes.data, C.c_void_p(d_y_ptr), C.byref(o)))

    def conv2d_fp8_ex(self, d_x_ptr: int, N, H, W, Cin, weight: np.ndarray, Cout, scale: Optional[np.ndarray] = None,
                      shift: Optional[np.ndarray] = None, act_scale: float = 8.0, quant: int = 0, d_res_ptr: int = 0, d_y_ptr: int = 0,
                      **opts) -> dict:
        """One 3x3 s1 p1 conv on e4m3 operands with the caller naming what runs (include/ltk.h: ltk_conv2d_fp8_ex; quant 0 = the
        program's rule, 1 = e4m3 MFMA, 2 = MX; `opts` = the fields of ltk_conv_opts, x_ld / x_coff in fp8 channels).  Returns the
        report of what was launched, as conv2d_f16_ex does."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32) if scale is not None else None
        sf = np.ascontiguousarray(shift, dtype=np.float32) if shift is not None else None
        o = _lib.ConvOpts(**{name: int(v) for name, v in opts.items()})
        rep = _lib.ConvReport()
        _lib.check(self._lib.ltk_conv2d_fp8_ex(
            self._h, C.c_void_p(d_x_ptr), N, H, W, Cin, w.ctypes.data, Cout, sc.ctypes.data if sc is not None else None,
            sf.ctypes.data if sf is not None else None, float(act_scale), int(quant), C.c_void_p(d_res_ptr) if d_res_ptr else None,
            C.c_void_p(d_y_ptr), C.byref(o), C.byref(rep)))
        return _conv_report_dict(rep)

    @staticmethod
    def conv_fp8_plan(N, H, W, Cin, Cout, quant: int = 0, has_res=False, k=3, stride=1, pad=1, transposed=False, out_pad=0, **opts) -> dict:
        """What conv2d_fp8_ex would report for this call, decided on the host alone (ltk_debug_conv_fp8_plan; no GPU needed).  k,
        stride, pad, transposed and out_pad exist to see the fp8 route refuse everything but 3x3 stride 1 pad 1."""
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        o = _lib.ConvOpts(**{name: int(v) for name, v in opts.items()})
        rep = _lib.ConvReport()
        _lib.check(_lib.load().ltk_debug_conv_fp8_plan(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, 1 if transposed else 0, out_pad,
                                                       int(quant), 1 if has_res else 0, C.byref(o), C.byref(rep)))
        return _conv_report_dict(rep)

    @staticmethod
    def conv3_fp8_variants() -> list:
        """Names of every fp8 conv3 instantiation the launch path can pick, e4m3 and MX (ltk_debug_conv3_fp8_variants); no GPU needed."""
        buf = C.create_string_buffer(8192)
        _lib.check(_lib.load().ltk_debug_conv3_fp8_variants(buf, len(buf)))
        return buf.value.decode().split()
