/* octpipe_render_modes.h -- included by octpipe.h (volume rendering), not meant to be included on its own.
 * The render mode that octpipe_render_volume does not take: it has a second pass (the surface map) and an entry point of its own,
 * octpipe_render_oct_depth.  octpipe.h's own enum stays the list of modes octpipe_render_volume accepts, which
 * tests/test_volume_render.py pins; this constant continues it. */
#ifndef OCTPIPE_RENDER_MODES_H
#define OCTPIPE_RENDER_MODES_H
enum {
	OCTPIPE_RENDER_OCT_DEPTH = 6
};
#endif /* OCTPIPE_RENDER_MODES_H */
