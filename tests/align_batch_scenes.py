"""Job lists for the batched alignment (include/trackdlo_hip.h: tdlo_align_depth_batch), built from the scenes of tests/align_ref.py -- no new statement: the
reference of a job is align_ref.align on its scene.  A job is a dict: name, s (the scene: D and p), kind (the view's layout: packed / pitched / bottom_up, as
align_ref.as_view_array lays it out), where ("host" / "device"), share (None, or the index of the job whose depth VIEW this job names under other params).

Each list is there for something it catches:
  one_5x7        J = 1, 5 x 7 -> 5 x 7: Pc = 35, the pack's tail is 3 words, the job is under one workgroup in both kernels
  tail1_first    J = 2, a 1 x 65 colour plane (tail 1) in FRONT of the upscale scene: the largest job comes second, so row 0's spare workgroups must leave
  mixed7         J = 7: upscale, downscale, border (Pd = 2240: no multiple of 256), rot80, ratio20 under max_footprint 64, f32, an all-zero 9 x 14 image
                 (every wave leaves before the counts; Pc = 126: Pc % 4 == 2); packed, pitched and bottom-up views, host and device views mixed
  same_view      one depth view under two params (the upscale scene, and the same view with max_footprint 1 and with another transform) beside a third job
  fused_among    the scene that tells a fused multiply-add from the statement, as one job among others: the no-FMA build flag of the batch unit
  full           three 480 x 640 depth images -> 720 x 1280 (the rope scene and two of its shifts): several workgroup rows of full-size jobs"""
import numpy as np

import align_ref as AR


def job(name, s, kind="packed", where="host", share=None):
    return dict(name=name, s=s, kind=kind, where=where, share=share)


def _all_zero():
    s = AR.same_camera(9, 14, 22)
    return dict(s, D=np.zeros((9, 14), np.uint16))


def _rope_shift(k):
    s = AR.scene_rope()
    return s if k == 0 else dict(s, D=np.ascontiguousarray(np.roll(s["D"], (17 * k, 53 * k), axis=(0, 1))))


def build():
    up = AR.scene_upscale()
    other_T = dict(up["p"], T=AR.transform(AR.rot("z", 2.0), (-0.01, 0.004, 0.003)))
    lists = dict(
        one_5x7=[job("5x7", AR.same_camera(5, 7, 31))],
        tail1_first=[job("1x65", AR.same_camera(1, 65, 32), where="device"), job("upscale", up, where="device")],
        mixed7=[job("upscale", up, "pitched", "device"), job("downscale", AR.scene_downscale(), "packed", "host"), job("border", AR.scene_border(), "bottom_up", "device"),
                job("rot80", AR.scene_rot80(), "pitched", "host"), job("ratio20_mf64", AR.scene_ratio20(64), "packed", "device"), job("f32", AR.scene_f32(), "bottom_up", "host"),
                job("all_zero", _all_zero(), "packed", "device")],
        same_view=[job("upscale", up, "pitched", "device"), job("upscale_mf1", dict(up, p=dict(up["p"], max_footprint=1)), "pitched", "device", share=0),
                   job("rot180", AR.scene_rot180(), "packed", "host"), job("upscale_T2", dict(up, p=other_T), "pitched", "device", share=0)],
        fused_among=[job("5x7", AR.same_camera(5, 7, 31), "bottom_up", "host"), job("fused", AR.scene_fused(), "packed", "device"), job("1x65", AR.same_camera(1, 65, 32), "pitched", "host")],
        full=[job(f"rope{k}", _rope_shift(k), "packed", "device" if k != 1 else "host") for k in range(3)],
    )
    return lists


LISTS = build()
SMALL = [n for n in LISTS if n != "full"]
_REF = {}


def reference(name):
    """[(plane, counts)] of a list's jobs by the statement, computed once and left unchanged"""
    if name not in _REF:
        out = []
        for j in LISTS[name]:
            A, n = AR.align(j["s"]["D"], j["s"]["p"])
            A.setflags(write=False)
            out.append((A, n))
        _REF[name] = out
    return _REF[name]


def properties():
    """what the docstring claims of the lists, as facts a test asserts"""
    m = LISTS["mixed7"]
    Pd = [j["s"]["D"].size for j in m]
    Pc = [j["s"]["p"]["rows_c"] * j["s"]["p"]["cols_c"] for j in m]
    t = LISTS["tail1_first"]
    return dict(one_tail=(LISTS["one_5x7"][0]["s"]["p"]["rows_c"] * LISTS["one_5x7"][0]["s"]["p"]["cols_c"]) % 4,
                tail1=(t[0]["s"]["p"]["rows_c"] * t[0]["s"]["p"]["cols_c"]) % 4, largest_second=t[1]["s"]["D"].size > t[0]["s"]["D"].size,
                Pd_off_block=any(p % 256 for p in Pd), Pc_mod4_2=any(p % 4 == 2 for p in Pc), kinds={j["kind"] for j in m}, wheres={j["where"] for j in m},
                zero=not m[6]["s"]["D"].any(), f32=m[5]["s"]["D"].dtype == np.float32, mf64=m[4]["s"]["p"]["max_footprint"] == 64)
