/*
 * gstmi355textoverlay.c -- GStreamer element `mi355textoverlay`: the drop-in for the `textoverlay` token in front of the encoder in
 * ceracoder's pipeline files (`textoverlay text='' valignment=top halignment=right font-desc="Monospace, 5" name=overlay ! queue !`).
 * The reference's control loop finds the element by its name `overlay` and rewrites its `text` property every 20 ms.
 *
 * It draws nothing and touches no buffer: a pass-through for any caps (no copy, no map).  When one of its properties has changed it
 * sends a serialized custom downstream event ("mi355-overlay") in front of the next buffer; `mi355h264enc` takes the text and style
 * from it and draws them on the GPU.  `font-desc` is accepted and ignored: the encoder has one built-in bitmap
 * font, sized by its own `overlay-scale`.
 */
#include <gst/gst.h>
#include <string.h>

GType gst_mi355_overlay_halign_type(void); /* gstmi355h264enc.c */
GType gst_mi355_overlay_valign_type(void);

typedef struct {
    GstElement parent;
    GstPad *sinkpad, *srcpad;
    /* properties (object lock) */
    gchar *text, *font_desc;
    gint halign, valign, xpad, ypad;
    gboolean shaded;
    gint dirty; /* atomic: a property was written since the last event */
} GstMi355TextOverlay;
typedef struct { GstElementClass parent_class; } GstMi355TextOverlayClass;

#define GST_MI355TEXTOVERLAY(o) (G_TYPE_CHECK_INSTANCE_CAST((o), gst_mi355textoverlay_get_type(), GstMi355TextOverlay))
G_DEFINE_TYPE(GstMi355TextOverlay, gst_mi355textoverlay, GST_TYPE_ELEMENT)

enum { PROP_0, PROP_TEXT, PROP_HALIGN, PROP_VALIGN, PROP_XPAD, PROP_YPAD, PROP_SHADED, PROP_FONT_DESC };

static GstStaticPadTemplate ov_sink_tmpl = GST_STATIC_PAD_TEMPLATE("sink", GST_PAD_SINK, GST_PAD_ALWAYS, GST_STATIC_CAPS_ANY);
static GstStaticPadTemplate ov_src_tmpl = GST_STATIC_PAD_TEMPLATE("src", GST_PAD_SRC, GST_PAD_ALWAYS, GST_STATIC_CAPS_ANY);

static void ov_set_property(GObject *obj, guint id, const GValue *val, GParamSpec *ps) {
    GstMi355TextOverlay *s = GST_MI355TEXTOVERLAY(obj);
    GST_OBJECT_LOCK(s);
    switch (id) {
    case PROP_TEXT: g_free(s->text); s->text = g_value_dup_string(val); break;
    case PROP_FONT_DESC: g_free(s->font_desc); s->font_desc = g_value_dup_string(val); break; /* kept for the getter only */
    case PROP_HALIGN: s->halign = g_value_get_enum(val); break;
    case PROP_VALIGN: s->valign = g_value_get_enum(val); break;
    case PROP_XPAD: s->xpad = g_value_get_int(val); break;
    case PROP_YPAD: s->ypad = g_value_get_int(val); break;
    case PROP_SHADED: s->shaded = g_value_get_boolean(val); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(obj, id, ps); break;
    }
    GST_OBJECT_UNLOCK(s);
    if (id != PROP_FONT_DESC) g_atomic_int_set(&s->dirty, 1);
}
static void ov_get_property(GObject *obj, guint id, GValue *val, GParamSpec *ps) {
    GstMi355TextOverlay *s = GST_MI355TEXTOVERLAY(obj);
    GST_OBJECT_LOCK(s);
    switch (id) {
    case PROP_TEXT: g_value_set_string(val, s->text ? s->text : ""); break;
    case PROP_FONT_DESC: g_value_set_string(val, s->font_desc ? s->font_desc : ""); break;
    case PROP_HALIGN: g_value_set_enum(val, s->halign); break;
    case PROP_VALIGN: g_value_set_enum(val, s->valign); break;
    case PROP_XPAD: g_value_set_int(val, s->xpad); break;
    case PROP_YPAD: g_value_set_int(val, s->ypad); break;
    case PROP_SHADED: g_value_set_boolean(val, s->shaded); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(obj, id, ps); break;
    }
    GST_OBJECT_UNLOCK(s);
}

static GstFlowReturn ov_chain(GstPad *pad, GstObject *parent, GstBuffer *buf) {
    GstMi355TextOverlay *s = GST_MI355TEXTOVERLAY(parent);
    (void)pad;
    if (g_atomic_int_compare_and_exchange(&s->dirty, 1, 0)) {
        GST_OBJECT_LOCK(s);
        GstStructure *st = gst_structure_new("mi355-overlay", "text", G_TYPE_STRING, s->text ? s->text : "", "halign", G_TYPE_INT, s->halign,
                                             "valign", G_TYPE_INT, s->valign > 2 ? 2 : s->valign, "xpad", G_TYPE_INT, s->xpad, "ypad", G_TYPE_INT, s->ypad,
                                             "shaded-background", G_TYPE_BOOLEAN, s->shaded, NULL);
        GST_OBJECT_UNLOCK(s);
        gst_pad_push_event(s->srcpad, gst_event_new_custom(GST_EVENT_CUSTOM_DOWNSTREAM, st));
    }
    return gst_pad_push(s->srcpad, buf);
}

static void ov_finalize(GObject *obj) {
    GstMi355TextOverlay *s = GST_MI355TEXTOVERLAY(obj);
    g_free(s->text); g_free(s->font_desc);
    G_OBJECT_CLASS(gst_mi355textoverlay_parent_class)->finalize(obj);
}

static void gst_mi355textoverlay_class_init(GstMi355TextOverlayClass *k) {
    GObjectClass *g = G_OBJECT_CLASS(k);
    GstElementClass *e = GST_ELEMENT_CLASS(k);
    const GParamFlags F = (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS | GST_PARAM_MUTABLE_PLAYING);
    g->set_property = ov_set_property; g->get_property = ov_get_property; g->finalize = ov_finalize;
    g_object_class_install_property(g, PROP_TEXT, g_param_spec_string("text", "Text", "Text for mi355h264enc downstream to draw (printable ASCII, newline starts a line, at most 255 bytes, no markup)", "", F));
    g_object_class_install_property(g, PROP_HALIGN, g_param_spec_enum("halignment", "Horizontal alignment", "Horizontal alignment of the text", gst_mi355_overlay_halign_type(), 2, F));
    g_object_class_install_property(g, PROP_VALIGN, g_param_spec_enum("valignment", "Vertical alignment", "Vertical alignment of the text (baseline: bottom)", gst_mi355_overlay_valign_type(), 0, F));
    g_object_class_install_property(g, PROP_XPAD, g_param_spec_int("xpad", "Horizontal padding", "Luma samples between the text box and the picture edge", 0, 8192, 16, F));
    g_object_class_install_property(g, PROP_YPAD, g_param_spec_int("ypad", "Vertical padding", "Luma samples between the text box and the picture edge", 0, 8192, 16, F));
    g_object_class_install_property(g, PROP_SHADED, g_param_spec_boolean("shaded-background", "Shaded background", "Darken the text box", FALSE, F));
    g_object_class_install_property(g, PROP_FONT_DESC, g_param_spec_string("font-desc", "Font description", "Accepted for textoverlay pipeline lines and ignored: the encoder draws its one built-in bitmap font (size: its overlay-scale)", "", F));
    gst_element_class_add_static_pad_template(e, &ov_sink_tmpl);
    gst_element_class_add_static_pad_template(e, &ov_src_tmpl);
    gst_element_class_set_static_metadata(e, "MI355X text overlay control", "Filter/Editor/Video",
        "Pass-through that hands its text and alignment to mi355h264enc downstream, which draws them on the GPU", "ceracoder-amd");
}
static void gst_mi355textoverlay_init(GstMi355TextOverlay *s) {
    s->text = NULL; s->font_desc = NULL; s->halign = 2; s->valign = 0; s->xpad = 16; s->ypad = 16; s->shaded = FALSE; s->dirty = 0;
    s->sinkpad = gst_pad_new_from_static_template(&ov_sink_tmpl, "sink");
    s->srcpad = gst_pad_new_from_static_template(&ov_src_tmpl, "src");
    gst_pad_set_chain_function(s->sinkpad, ov_chain);
    /* caps, allocation and scheduling queries and every event pass straight through */
    GST_PAD_SET_PROXY_CAPS(s->sinkpad); GST_PAD_SET_PROXY_ALLOCATION(s->sinkpad); GST_PAD_SET_PROXY_SCHEDULING(s->sinkpad);
    GST_PAD_SET_PROXY_CAPS(s->srcpad); GST_PAD_SET_PROXY_SCHEDULING(s->srcpad);
    gst_element_add_pad(GST_ELEMENT(s), s->sinkpad);
    gst_element_add_pad(GST_ELEMENT(s), s->srcpad);
}
