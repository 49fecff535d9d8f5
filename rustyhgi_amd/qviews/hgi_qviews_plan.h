// Requantize view lists (hgi_qviews_requant_dev, include/hgi_qviews.h): the launch's whole judgement, as one function that
// returns a status and a message.  The PLAN of a list is the view lists' (../views/hgi_views_plan.h, hgi_views_plan), as it
// stands: `src` is the side that is read, the page rule holds per entry on the source span, the 32-bit bound covers both
// pitches, outputs are pairwise disjoint, no output meets an input (in place is refused with that: requantize's own rule) and
// inputs may overlap.  This header adds no blob, no record, no magic and no aliasing code; it takes views_info_consistent and
// view_args from that header and puts requantize's table rule (../requant/hgi_requant.hip: the identity table is refused, the
// result is the source) behind the launch rules of hgi_views_encode_dev.
// Plain C++, no HIP: tests/cpp/test_qviews_plan.cpp runs it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hgi_qviews.h"
#include "../views/hgi_views_plan.h"

namespace hgi {

enum QViewsVerdict {
    kQViewsLaunch = 0,            // every rule holds: k / up are set
    kQViewsEmpty,                 // a plan of no frame: HGI_OK, nothing launched
    // HGI_EINVAL
    kQViewsInfoNull, kQViewsInfo, kQViewsPlanNull, kQViewsPlanAlign, kQViewsLutNull, kQViewsLevelsRange, kQViewsInterp,
    // HGI_EUNSUPPORTED
    kQViewsLevels, kQViewsIdentity,
};

struct QViewsJudged {
    hgi_status status;
    QViewsVerdict verdict;
    uint32_t k, up;               // how the pyramid is split between the tile and the cone (kQViewsLaunch only)
    char text[256];               // the refusal's message; empty on HGI_OK
};

inline bool qviews_identity(const uint8_t *lut)
{
    bool ident = true;
    for (int i = 0; i < 256; ++i) ident = ident && lut[i] == i;
    return ident;
}

// The rules of the launch entry in the header's order.  No HIP call, no allocation; `d_plan` is judged as an address only and
// `lut` is read (256 bytes of host memory) only behind every other rule.
inline QViewsJudged qviews_judge(const void *d_plan, const hgi_views_info *info, uint32_t levels, hgi_interp interp, const uint8_t *lut)
{
    QViewsJudged j;
    j.status = HGI_OK;
    j.verdict = kQViewsEmpty;
    j.k = j.up = 0;
    j.text[0] = 0;
    // a plan of no frame succeeds and does nothing, whatever the other arguments
    if (info && info->magic == HGI_VIEWS_MAGIC && info->count == 0 && views_info_consistent(*info)) return j;
    auto refuse = [&](hgi_status st, QViewsVerdict v) -> QViewsJudged & {
        j.status = st;
        j.verdict = v;
        return j;
    };
    // ---- HGI_EINVAL ----
    if (!info) {
        snprintf(j.text, sizeof(j.text), "info is NULL");
        return refuse(HGI_EINVAL, kQViewsInfoNull);
    }
    if (!views_info_consistent(*info)) {
        snprintf(j.text, sizeof(j.text), "info is not what hgi_views_plan wrote (magic, sizes and offsets against the count %u, block count)", info->count);
        return refuse(HGI_EINVAL, kQViewsInfo);
    }
    if (!d_plan) {
        snprintf(j.text, sizeof(j.text), "d_plan is NULL");
        return refuse(HGI_EINVAL, kQViewsPlanNull);
    }
    if (reinterpret_cast<uintptr_t>(d_plan) % 16 != 0) {
        snprintf(j.text, sizeof(j.text), "d_plan is not 16-byte aligned");
        return refuse(HGI_EINVAL, kQViewsPlanAlign);
    }
    if (!lut) {
        snprintf(j.text, sizeof(j.text), "lut is NULL");
        return refuse(HGI_EINVAL, kQViewsLutNull);
    }
    if (levels > 31) {
        snprintf(j.text, sizeof(j.text), "levels %u out of range 0..=31", levels);
        return refuse(HGI_EINVAL, kQViewsLevelsRange);
    }
    if (interp != HGI_INTERP_LEFTTOP && interp != HGI_INTERP_CROSSED) {
        snprintf(j.text, sizeof(j.text), "interpolator %d unknown (0 = LeftTop, 1 = Crossed)", (int)interp);
        return refuse(HGI_EINVAL, kQViewsInterp);
    }
    // ---- HGI_EUNSUPPORTED ----
    if (levels == 0 || levels > 8) {
        snprintf(j.text, sizeof(j.text), "levels %u: one launch serves 1..=8 levels (compose one requantize call per view)", levels);
        return refuse(HGI_EUNSUPPORTED, kQViewsLevels);
    }
    if (qviews_identity(lut)) {
        snprintf(j.text, sizeof(j.text), "the identity table re-codes a grid into itself: copy the source (no kernel is built for it)");
        return refuse(HGI_EUNSUPPORTED, kQViewsIdentity);
    }
    j.verdict = kQViewsLaunch;
    split_levels(levels, &j.k, &j.up);
    return j;
}

}  // namespace hgi
